// ttx_tt_bf16q.hip -- the bf16 inference forward of a FOUR-core TT table, all three products on the bf16 MFMA in matrix-chain
// order: row = (core_0 core_1) (core_2 core_3).  The fp32 four-core route writes the merged last cores M of every lookup to the
// plan in HBM and runs a three-core kernel over them; here M of a lookup (<= 64 x 32 values) lives in LDS beside x_0 and nothing
// of a lookup goes to memory except its row.  include/ttx.h "bf16 inference forward, four cores"; DESIGN.md section 4.24.
//
// A work-group takes one pivot chunk of the plan (chunk_rec: <= MC lookups of ONE core-1 slice; lrec = {n, sid_0, sid_2, sid_3})
// and walks it in passes of SC lookups.  Every product is TRANSPOSED, so that a lane's four accumulators are contiguous outputs:
//   phase 1a   x_0^T into X: ttx_tt_bf16m.hip's product 1.  M = the core-1 columns (b, k2), N = the pass's rows (j, a), K = k1.
//              The gathered core-0 fragments stay in registers for the pass, the core-1 fragments are streamed one M tile ahead.
//              A lane's accumulators are k2 = 16 t + 4 (l >> 4) .. + 3 of row (j, a) = l & 15: ONE 8-byte store to X[j][a][b][k2].
//   phase 1b   M^T into Y: per (lookup j, c, k2 tile t) an MFMA with M = k2 = 16 t + (l & 15), N = d = l & 15, K = k3.  A = one
//              16-byte load per K block from core 2 packed [r2 q2][K3p], B = one from core 3 packed [16][K3p].  A lane's
//              accumulators are k2 = 16 t + 4 (l >> 4) .. + 3 of column (c, d): ONE 8-byte store to Y[j][(c, d)][k2], d < q3.
//              The items go to the waves in units of 8 / K3B items of one lookup, whose loads are issued together, one unit
//              ahead of the MFMAs: every lookup has its own core-2 slice, and these loads are the kernel's memory traffic.
//              1a and 1b are independent: a wave issues 1a's gathers, works through its share of 1b while they travel, then runs
//              its share of 1a.  ONE barrier follows both.
//   phase 2    row^T per lookup: M = (c, d) (Q23P / 16 tiles), N = 16 rows (a, b), K = k2, both fragments ds_read_b128 (A from Y,
//              B from X).  A lane holds (c, d) = 16 mq + 4 (l >> 4) .. + 3 of row (a, b) = l & 15: one 16-byte store to
//              rows[lrec.x] (scalar stores where q2 q3 % 4 != 0).
// X (bf16): row (j, a, b) at ((j q0 + a) AS + b S) bytes, S = 2 (K2p + 8) (S / 16 odd: the 16 rows of a phase-2 read fall on 16
// different 16-byte bank groups), AS = q1 S (+ 16 where q1 is even).  Y (bf16): row (j, (c, d)) at (j Q23P + (c, d)) S bytes.
// Columns [16 ceil(r2 / 16), K2p) of both and the rows [q2 q3, Q23P) of Y are written by nobody else: zeroed once per work-group.
// Rows go out in ORIGINAL lookup order (lrec.x), each element written once: no atomics, bit-identical from run to run.
#include "ttx_internal.h"

namespace ttx {
namespace {

constexpr int kBqThreads = 256;
constexpr int kBqWaves = kBqThreads / kWave;
constexpr int kBqNT = 4;                // N tiles (16 rows (lookup, a)) of a pass, at most
constexpr int kBqRows = 16 * kBqNT;
constexpr int kBqMaxRank = 64;          // r1, r2, r3
constexpr int kBqMaxQ23 = 32;           // q2 q3
constexpr int kBqLdsGoal = 80 * 1024;   // LDS of a work-group that leaves room for two per CU
constexpr int kBqLdsMax = 160 * 1024;   // LDS of a work-group
constexpr int kBqRecBytes = 2 * 16 * kBqRows;  // two sets of lookup records (int4), used by alternate passes

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernels need of a geometry (host-derived; travels by value)
struct BqShape {
  int q0, q1, q2, q3, r1, r2, r3;
  int K1p, K2p, K3p;  // r1, r2, r3 padded to the MFMA's K (32)
  int N1, N1p;        // q1 r2 columns of x_0, padded to 16 (the packed core 1)
  int Q23, Q23P;      // q2 q3 columns (c, d) of M, padded to 16
  int MT;             // k2 tiles: ceil(r2 / 16)
  int R, NT2;         // rows (a, b) of a lookup, N tiles of a lookup in phase 2
  int S, AS, YS;      // bytes between rows b / rows a of X (S: between rows (c, d) of Y too), Y of one lookup
  int SC;             // lookups of a pass
  int D;
  int Sl[4];          // slices of core t
  int pe[4];          // packed bf16 elements of a slice of core t
  int lds_bytes;
};

// host-only: no Dims, no device.  false: not a shape of this kernel.
bool bq_shape(const ttx_geom* g, BqShape* o) {
  if (!g || g->T != 4 || g->num_tables <= 0 || g->r[0] != 1 || g->r[4] != 1) return false;
  for (int t = 0; t < 4; ++t)
    if (g->q[t] <= 0) return false;
  for (int t = 1; t < 4; ++t)
    if (g->r[t] <= 0 || g->r[t] > kBqMaxRank) return false;
  if (g->q[0] > 16 || g->q[1] > 64 || g->q[3] > 16 || g->q[2] > kBqMaxQ23 || g->q[2] * g->q[3] > kBqMaxQ23) return false;
  BqShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.q3 = g->q[3];
  s.r1 = g->r[1]; s.r2 = g->r[2]; s.r3 = g->r[3];
  s.K1p = (s.r1 + 31) / 32 * 32;
  s.K2p = (s.r2 + 31) / 32 * 32;
  s.K3p = (s.r3 + 31) / 32 * 32;
  s.N1 = s.q1 * s.r2;
  s.N1p = (s.N1 + 15) / 16 * 16;
  s.Q23 = s.q2 * s.q3;
  s.Q23P = (s.Q23 + 15) / 16 * 16;
  s.MT = (s.r2 + 15) / 16;
  s.R = s.q0 * s.q1;
  s.NT2 = (s.R + 15) / 16;
  s.S = 2 * (s.K2p + 8);                         // (K2p / 8 is a multiple of 4: S / 16 = K2p / 8 + 1 is odd)
  s.AS = s.q1 * s.S + (s.q1 % 2 == 0 ? 16 : 0);  // (q1 odd: q1 S / 16 is odd already)
  s.YS = s.Q23P * s.S;
  s.D = s.R * s.Q23;
  s.pe[0] = s.q0 * s.K1p;
  s.pe[1] = s.N1p * s.K1p;
  s.pe[2] = s.r2 * s.q2 * s.K3p;
  s.pe[3] = 16 * s.K3p;
  const int one = s.q0 * s.AS + s.YS;  // X + Y of one lookup
  if (one + kBqRecBytes > kBqLdsMax) return false;
  s.SC = kBqRows / s.q0;
  while (s.SC > 1 && s.SC * one + kBqRecBytes > kBqLdsGoal) --s.SC;
  s.lds_bytes = s.SC * one + kBqRecBytes;
  if (o) *o = s;
  return true;
}

// ---------------------------------------------------------------- pack -----
// float -> bf16, round to nearest even; NaN -> 0x7FC0 (what tensor.to(torch.bfloat16) computes)
__device__ __forceinline__ unsigned short bf16_rne(float f) {
  const unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (unsigned short)0x7FC0;
  return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// cores 0 and 1: the packed layout of ttx_tt_bf16.hip; core 2: [r2 q2][K3p], the natural order with k3 padded; core 3:
// [16][K3p], column d of the slice [r3][q3] with its k3 index contiguous (include/ttx.h)
__global__ __launch_bounds__(256) void pack_bf16q_kernel(int t, int pe, BqShape sh, long long total, const float* __restrict__ src,
                                                         unsigned short* __restrict__ dst) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long sl = e / pe;
    const int w = (int)(e - sl * pe);
    long long at = -1;  // the fp32 element, -1: padding
    if (t == 0) {        // [q0][K1p]
      const int a = w / sh.K1p, k = w - a * sh.K1p;
      if (k < sh.r1) at = sl * (sh.q0 * sh.r1) + a * sh.r1 + k;
    } else if (t == 1) {  // [N1p][K1p]: column n = b r2 + k2 of the slice [r1][q1][r2], its K index contiguous
      const int n = w / sh.K1p, k = w - n * sh.K1p;
      if (n < sh.N1 && k < sh.r1) at = sl * ((long long)sh.r1 * sh.N1) + (long long)k * sh.N1 + n;
    } else if (t == 2) {  // [r2 q2][K3p]: row (k2, c) of the slice [r2][q2][r3]
      const int rq = w / sh.K3p, k = w - rq * sh.K3p;
      if (k < sh.r3) at = sl * ((long long)sh.r2 * sh.q2 * sh.r3) + (long long)rq * sh.r3 + k;
    } else {              // [16][K3p]: column d of the slice [r3][q3], its K index contiguous
      const int d = w / sh.K3p, k = w - d * sh.K3p;
      if (d < sh.q3 && k < sh.r3) at = sl * (sh.r3 * sh.q3) + k * sh.q3 + d;
    }
    dst[e] = at >= 0 ? bf16_rne(src[at]) : (unsigned short)0;
  }
}

// ---------------------------------------------------------------- rows -----
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// two fp32 -> two bf16 in one dword, round to nearest even (gfx950: one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// the A fragments of phase 1a's M tile mt = b MT + t: column k2 = 16 t + (l & 15) of q1 block b, k = 8 (l >> 4) .. + 7 of every
// 32; zero where the tile or the column does not exist (nothing is read there)
template <int KB>
__device__ __forceinline__ void load_a1(uint4 (&af)[KB], const unsigned short* __restrict__ base1, int mt, int nm, const BqShape& sh,
                                        int li, int lg) {
  const int b = mt / sh.MT;
  const int k2 = 16 * (mt - b * sh.MT) + li;
  const bool ok = mt < nm && k2 < sh.r2;
  const unsigned short* ap = base1 + (size_t)(ok ? b * sh.r2 + k2 : 0) * (KB * 32) + 8 * lg;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) af[kb] = ok ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
}

// the fragments of phase 1b's unit u = j NG + g: the G items (c, t) = g G .. + G - 1 of lookup j, in the order c MT + t.  B = row
// d = l & 15 of the lookup's core-3 slice (rows q3 .. 15 are the pack's zeros), once for the unit; A of an item = row (k2 = 16 t +
// (l & 15), c) of its core-2 slice; k = 8 (l >> 4) .. + 7 of every 32.  Zero where the unit, the item or the row k2 does not exist
// (nothing is read there).  All G K3B + K3B loads are issued together: they are what covers one another's latency.
template <int K3B, int G>
__device__ __forceinline__ void load_ab3(uint4 (&af)[G][K3B], uint4 (&bf)[K3B], const int4* I, const unsigned short* __restrict__ c2,
                                         const unsigned short* __restrict__ c3, int u, int nu, int NG, const BqShape& sh, int li,
                                         int lg) {
  const bool live = u < nu;
  const int j = live ? u / NG : 0;
  const int item0 = (u - j * NG) * G;
  const int4 rec = I[j];
  const unsigned short* bp = c3 + (size_t)rec.w * sh.pe[3] + li * (K3B * 32) + 8 * lg;
#pragma unroll
  for (int kb = 0; kb < K3B; ++kb) bf[kb] = live ? *(const uint4*)(bp + kb * 32) : make_uint4(0, 0, 0, 0);
  const unsigned short* a0 = c2 + (size_t)rec.z * sh.pe[2] + 8 * lg;
  int c = item0 / sh.MT, t = item0 - c * sh.MT;
#pragma unroll
  for (int i = 0; i < G; ++i) {
    const int k2 = 16 * t + li;
    const bool ok = live && c < sh.q2 && k2 < sh.r2;
    const unsigned short* ap = a0 + (size_t)(ok ? k2 * sh.q2 + c : 0) * (K3B * 32);
#pragma unroll
    for (int kb = 0; kb < K3B; ++kb) af[i][kb] = ok ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
    if (++t == sh.MT) {
      t = 0;
      ++c;
    }
  }
}

template <int KB, int K2B, int K3B, int MQ>  // KB = K1p / 32, K2B = K2p / 32, K3B = K3p / 32, MQ = Q23P / 16
__global__ __launch_bounds__(kBqThreads) void tt_rows_bf16q_kernel(const int4* __restrict__ chunk_rec, const int4* __restrict__ lrec,
                                                                   int nnz, BqShape sh, const unsigned short* __restrict__ c0,
                                                                   const unsigned short* __restrict__ c1,
                                                                   const unsigned short* __restrict__ c2,
                                                                   const unsigned short* __restrict__ c3, float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int4* Irec = (int4*)smem;                          // [2][64] records of a pass: {lookup n, slices of cores 0, 2, 3}
  unsigned char* X = smem + kBqRecBytes;             // [SC q0] row groups of AS bytes: x_0 of the pass, bf16
  unsigned char* Y = X + (size_t)sh.SC * sh.q0 * sh.AS;  // [SC][Q23P] rows of S bytes: M^T of the pass, bf16
  const int4 cr = chunk_rec[blockIdx.x];
  if (cr.z <= 0) return;
  // (the plan is trusted for its order, not for memory safety: every index it hands over is clamped)
  const int s = clampi(cr.x, 0, sh.Sl[1] - 1);
  const int start = clampi(cr.y, 0, nnz);
  const int len = min(cr.z, nnz - start);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int li = lane & 15, lg = lane >> 4;
  const int K1p = KB * 32, K2p = K2B * 32;
  const unsigned short* base1 = c1 + (size_t)s * sh.pe[1];
  const int nm = sh.q1 * sh.MT;  // M tiles of phase 1a
  // what phase 1 never writes (a stale NaN there times the other operand's zero is a NaN); visible after the first barrier below:
  // the 16 bf16 at [16 MT, K2p) of every row of X ...
  if (16 * sh.MT < K2p) {
    const int nrow = sh.SC * sh.R;
    for (int e = tid; e < 2 * nrow; e += kBqThreads) {
      const int row = e >> 1;
      const int ja = row / sh.q1;
      *(uint4*)(X + (size_t)ja * sh.AS + (row - ja * sh.q1) * sh.S + 32 * sh.MT + 16 * (e & 1)) = make_uint4(0, 0, 0, 0);
    }
  }
  // ... and of every row of Y, and the whole of its rows (c, d) in [Q23, Q23P)
  if (16 * sh.MT < K2p || sh.Q23 < 16 * MQ) {
    const int npiece = sh.SC * 16 * MQ * (K2p / 8);  // 16-byte pieces of the rows' K2p columns
    for (int e = tid; e < npiece; e += kBqThreads) {
      const int row = e / (K2p / 8), piece = e - row * (K2p / 8);
      if ((row & (16 * MQ - 1)) >= sh.Q23 || piece >= 2 * sh.MT)
        *(uint4*)(Y + (size_t)row * sh.S + 16 * piece) = make_uint4(0, 0, 0, 0);
    }
  }
  int4* I = Irec;
  for (int j0 = 0; j0 < len; j0 += sh.SC) {
    const int lenS = min(sh.SC, len - j0);
    const int rowsS = lenS * sh.q0;
    I = I == Irec ? Irec + kBqRows : Irec;  // (a wave still in the last pass's phase 2 reads the other set)
    if (tid < lenS) {
      int4 r = lrec[start + j0 + tid];
      r.x = clampi(r.x, 0, nnz - 1);
      r.y = clampi(r.y, 0, sh.Sl[0] - 1);
      r.z = clampi(r.z, 0, sh.Sl[2] - 1);
      r.w = clampi(r.w, 0, sh.Sl[3] - 1);
      I[tid] = r;
    }
    __syncthreads();  // the records are there; every wave has left the last pass: its X and Y are read
    // ---- phase 1
    {
      // 1a's B fragments of the pass (row (j, a) = 16 nt + (l & 15), k = 8 (l >> 4) .. + 7) and its first A fragments: issued
      // here, used behind 1b
      uint4 bf[kBqNT][KB];
#pragma unroll
      for (int nt = 0; nt < kBqNT; ++nt) {
        const int m = nt * 16 + li;
        const bool live = m < rowsS;
        const int j = live ? m / sh.q0 : 0;
        const int a = live ? m - j * sh.q0 : 0;
        const unsigned short* bp = c0 + (size_t)I[j].y * sh.pe[0] + a * K1p + 8 * lg;
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) bf[nt][kb] = live ? *(const uint4*)(bp + kb * 32) : make_uint4(0, 0, 0, 0);
      }
      uint4 af[KB];
      load_a1<KB>(af, base1, wave, nm, sh, li, lg);
      // 1b: units of G items (c, t) of one lookup over the waves, the next unit's fragments beside this one's MFMAs
      {
        constexpr int G = 8 / K3B;
        const int NG = (sh.q2 * sh.MT + G - 1) / G;
        const int nu = lenS * NG;
        uint4 a3[G][K3B], b3[K3B];
        load_ab3<K3B, G>(a3, b3, I, c2, c3, wave, nu, NG, sh, li, lg);
        for (int u = wave; u < nu; u += kBqWaves) {
          uint4 a3n[G][K3B], b3n[K3B];
          load_ab3<K3B, G>(a3n, b3n, I, c2, c3, u + kBqWaves, nu, NG, sh, li, lg);
          const int j = u / NG;
          const int item0 = (u - j * NG) * G;
          int c = item0 / sh.MT, t = item0 - c * sh.MT;
          unsigned char* ycol = Y + (size_t)(j * 16 * MQ + li) * sh.S + 8 * lg;
#pragma unroll
          for (int i = 0; i < G; ++i) {
            if (c < sh.q2) {  // (wave-uniform)
              f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int kb = 0; kb < K3B; ++kb)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a3[i][kb]), __builtin_bit_cast(bf16x8, b3[kb]),
                                                              acc, 0, 0, 0);
              if (li < sh.q3)  // (row (c, d) < Q23 of lookup j < SC, columns 16 t + 4 lg + 3 < 16 MT <= K2p: inside Y)
                *(uint2*)(ycol + (size_t)c * sh.q3 * sh.S + 32 * t) = make_uint2(pk_bf16(acc[0], acc[1]), pk_bf16(acc[2], acc[3]));
            }
            if (++t == sh.MT) {
              t = 0;
              ++c;
            }
          }
#pragma unroll
          for (int kb = 0; kb < K3B; ++kb) b3[kb] = b3n[kb];
#pragma unroll
          for (int i = 0; i < G; ++i)
#pragma unroll
            for (int kb = 0; kb < K3B; ++kb) a3[i][kb] = a3n[i][kb];
        }
      }
      // 1a: the M tiles over the waves
      for (int mt = wave; mt < nm; mt += kBqWaves) {
        uint4 an[KB];
        load_a1<KB>(an, base1, mt + kBqWaves, nm, sh, li, lg);  // (travels beside this tile's MFMAs)
        const int b = mt / sh.MT;
        unsigned char* xcol = X + b * sh.S + 2 * (16 * (mt - b * sh.MT) + 4 * lg);  // (16 t + 4 lg + 3 < 16 MT <= K2p)
#pragma unroll
        for (int nt = 0; nt < kBqNT; ++nt) {
          if (nt * 16 < rowsS) {  // (wave-uniform)
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < KB; ++kb)
              acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kb]), __builtin_bit_cast(bf16x8, bf[nt][kb]),
                                                            acc, 0, 0, 0);
            const int m = nt * 16 + li;
            if (m < rowsS)  // (m < SC q0: inside X)
              *(uint2*)(xcol + (size_t)m * sh.AS) = make_uint2(pk_bf16(acc[0], acc[1]), pk_bf16(acc[2], acc[3]));
          }
        }
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) af[kb] = an[kb];
      }
    }
    __syncthreads();  // X and Y of the pass are whole
    // ---- phase 2: tiles (lookup j, 16 rows (a, b)) over the waves; the lookup's M^T fragments reloaded from Y when j changes
    {
      uint4 yf[MQ][K2B];
      int jc = -1;
      const int ntile = lenS * sh.NT2;
      for (int tix = wave; tix < ntile; tix += kBqWaves) {
        const int j = tix / sh.NT2;
        const int4 rec = I[j];
        if (j != jc) {  // (wave-uniform) row (c, d) = 16 mq + (l & 15) of the lookup's Y, k2 = 8 (l >> 4) .. + 7 of every 32
          jc = j;
          const unsigned char* yr = Y + (size_t)(j * 16 * MQ + li) * sh.S + 16 * lg;
#pragma unroll
          for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
            for (int kb = 0; kb < K2B; ++kb) yf[mq][kb] = *(const uint4*)(yr + (size_t)mq * 16 * sh.S + 64 * kb);
        }
        const int rho = 16 * (tix - j * sh.NT2) + li;  // this lane's row (a, b) of the lookup
        const int rr = min(rho, sh.R - 1);              // (a row past the lookup's last reads the last: no read leaves X)
        const int a = rr / sh.q1;
        const unsigned char* xr = X + (size_t)(j * sh.q0 + a) * sh.AS + (rr - a * sh.q1) * sh.S + 16 * lg;
        f32x4 acc[MQ];
#pragma unroll
        for (int mq = 0; mq < MQ; ++mq) acc[mq] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < K2B; ++kb) {
          const uint4 xv = *(const uint4*)(xr + 64 * kb);
#pragma unroll
          for (int mq = 0; mq < MQ; ++mq)
            acc[mq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, yf[mq][kb]), __builtin_bit_cast(bf16x8, xv),
                                                              acc[mq], 0, 0, 0);
        }
        if (rho < sh.R) {
          float* out = rows + (size_t)rec.x * sh.D + (size_t)rho * sh.Q23 + 4 * lg;
#pragma unroll
          for (int mq = 0; mq < MQ; ++mq) {
            const int cd = 16 * mq + 4 * lg;
            if ((sh.Q23 & 3) == 0) {  // (D % 4 == 0 and rows 16-byte aligned: the piece is too; cd < Q23 then cd + 3 < Q23)
              if (cd < sh.Q23) *(float4*)(out + 16 * mq) = make_float4(acc[mq][0], acc[mq][1], acc[mq][2], acc[mq][3]);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (cd + i < sh.Q23) out[16 * mq + i] = acc[mq][i];
            }
          }
        }
      }
    }
    // (the next pass's first barrier stands between these reads of X / Y and its stores)
  }
}

template <int KB, int K2B, int K3B, int MQ>
int launch_rows(const Plan& P, int nnz, const BqShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  const void* fn = (const void*)tt_rows_bf16q_kernel<KB, K2B, K3B, MQ>;
  if (sh.lds_bytes > 48 * 1024) {
    const int rc = allow_dynamic_lds(fn, sh.lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tt_rows_bf16q_kernel<KB, K2B, K3B, MQ>), dim3(P.max_chunks), dim3(kBqThreads), sh.lds_bytes, st,
                     (const int4*)P.chunk_rec, (const int4*)P.lrec, nnz, sh, pc[0], pc[1], pc[2], pc[3], rows);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

template <int KB, int K2B, int K3B>
int launch_rows_mq(const Plan& P, int nnz, const BqShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  return sh.Q23P == 16 ? launch_rows<KB, K2B, K3B, 1>(P, nnz, sh, pc, rows, st) : launch_rows<KB, K2B, K3B, 2>(P, nnz, sh, pc, rows, st);
}

template <int KB, int K2B>
int launch_rows_k3(const Plan& P, int nnz, const BqShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  return sh.K3p == 32 ? launch_rows_mq<KB, K2B, 1>(P, nnz, sh, pc, rows, st) : launch_rows_mq<KB, K2B, 2>(P, nnz, sh, pc, rows, st);
}

template <int KB>
int launch_rows_k2(const Plan& P, int nnz, const BqShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  return sh.K2p == 32 ? launch_rows_k3<KB, 1>(P, nnz, sh, pc, rows, st) : launch_rows_k3<KB, 2>(P, nnz, sh, pc, rows, st);
}

}  // namespace
}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_rows_bf16q_supported(const ttx_geom* g) { return bq_shape(g, nullptr) ? 1 : 0; }

int64_t ttx_tt_pack_bf16q_elems(const ttx_geom* g, int32_t t) {
  BqShape sh;
  if (!bq_shape(g, &sh) || t < 0 || t > 3) return 0;
  long long S = 0;
  if (g->p_tables && g->num_tables > 1) {
    for (int k = 0; k < g->num_tables; ++k) {
      const int pk = g->p_tables[(size_t)k * 4 + t];
      if (pk <= 0) return 0;
      S += pk;
    }
  } else {
    if (g->p[t] <= 0) return 0;
    S = (long long)g->num_tables * g->p[t];
  }
  return S * sh.pe[t];
}

int ttx_tt_pack_bf16q(const ttx_geom* g, int32_t t, const float* core_f32, void* packed, ttx_stream_t stream) {
  BqShape sh;
  if (!g) TTX_FAIL(TTX_EINVAL, "pack_bf16q: geometry is NULL");
  if (!bq_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED,
             "pack_bf16q: not a shape of the four-core bf16 kernel (T = 4, ranks <= %d, q2 q3 <= %d, x_0 and M of a lookup in LDS)",
             kBqMaxRank, kBqMaxQ23);
  if (t < 0 || t > 3) TTX_FAIL(TTX_EINVAL, "pack_bf16q: core %d out of range", t);
  const long long total = ttx_tt_pack_bf16q_elems(g, t);
  if (total <= 0) TTX_FAIL(TTX_EINVAL, "pack_bf16q: p must be > 0");
  if (!core_f32 || !packed) TTX_FAIL(TTX_EINVAL, "pack_bf16q: NULL input / output");
  if ((((uintptr_t)core_f32) & 3) || (((uintptr_t)packed) & 15))
    TTX_FAIL(TTX_EINVAL, "pack_bf16q: core_f32 must be 4-byte, packed 16-byte aligned");
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(pack_bf16q_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (int)t,
                     sh.pe[t], sh, total, core_f32, (unsigned short*)packed);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

size_t ttx_tt_rows_bf16q_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz) {
  (void)D;
  Dims d;
  if (!bq_shape(g, nullptr) || nnz < 0 || make_dims(g, &d) != TTX_OK) return 0;
  return plan_bytes(d, nnz) + 256;
}

int ttx_tt_rows_bf16q(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                      const void* const* packed_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                      ttx_stream_t stream) {
  Dims d;
  int rc = make_dims(g, &d);
  if (rc) return rc;
  BqShape sh;
  if (!bq_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED,
             "tt_rows_bf16q: not a shape of the four-core bf16 kernel (T = 4, ranks <= %d, q0 <= 16, q1 <= 64, q3 <= 16, q2 q3 <= %d, "
             "x_0 and M of a lookup in LDS)",
             kBqMaxRank, kBqMaxQ23);
  if (D != d.D) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16q: D=%d does not match prod(q)=%d", D, d.D);
  if (nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16q: nnz=%lld out of range", (long long)nnz);
  if (nnz == 0) return TTX_OK;
  if (!packed_cores || !packed_cores[0] || !packed_cores[1] || !packed_cores[2] || !packed_cores[3] || !rows)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16q: NULL packed cores / rows");
  if ((((uintptr_t)packed_cores[0]) | ((uintptr_t)packed_cores[1]) | ((uintptr_t)packed_cores[2]) | ((uintptr_t)packed_cores[3]) |
       ((uintptr_t)rows)) & 15)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16q: packed cores and rows must be 16-byte aligned");
  if (!plan && !indices) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16q: NULL indices (and no plan)");
  if (choose_chunk(d, nnz) <= 0) TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16q: no lookup plan for this shape");
  for (int t = 0; t < 4; ++t) sh.Sl[t] = d.S[t];
  hipStream_t st = (hipStream_t)stream;
  Plan P;
  if (plan) {
    P = carve_plan(d, nnz, (void*)plan);
  } else {
    const size_t pb = plan_bytes(d, nnz);
    if (!workspace || workspace_bytes < pb) TTX_FAIL(TTX_EWORKSPACE, "tt_rows_bf16q: workspace too small: %zu < %zu", workspace_bytes, pb);
    P = carve_plan(d, nnz, workspace);
    rc = plan_build(d, nnz, indices, tableidx, nullptr, P, st);
    if (rc) return rc;
  }
  const unsigned short* pc[4] = {(const unsigned short*)packed_cores[0], (const unsigned short*)packed_cores[1],
                                 (const unsigned short*)packed_cores[2], (const unsigned short*)packed_cores[3]};
  return sh.K1p == 32 ? launch_rows_k2<1>(P, (int)nnz, sh, pc, rows, st) : launch_rows_k2<2>(P, (int)nnz, sh, pc, rows, st);
}

}  // extern "C"
