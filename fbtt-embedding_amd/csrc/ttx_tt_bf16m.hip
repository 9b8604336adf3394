// ttx_tt_bf16m.hip -- the bf16 inference forward of a three-core TT table with BOTH products on the bf16 MFMA: q2 up to 32, the
// row widths (D >= 640 by the default factorings) whose last core the other two bf16 kernels refuse (their VALU tail stops at
// q2 <= 8).  Same plan, same contract and numerics bound, the FIRST kernel to use the bound's 2^-8 term (x_0 is rounded once to
// bf16): include/ttx.h "bf16 inference forward, MFMA tail"; DESIGN.md section 4.21.
//
// A work-group takes one pivot chunk of the plan (chunk_rec: <= MC lookups of ONE core-1 slice) and walks it in passes of SC
// lookups (SC q0 <= 64 rows (lookup, a), and the pass's x_0 within the LDS goal).  Both products are TRANSPOSED, so that a lane's
// four accumulators are contiguous outputs:
//   product 1   x_0^T: M = the core-1 columns (b, k2), N = the pass's rows (j, a).  B fragments (the gathered core-0 rows: <= 4 N
//               tiles x KB 16-byte loads per lane) stay in registers for the pass; the A fragments (the packed core-1 slice, row
//               l & 15 = column (b, k2), k = 8 (l >> 4) .. + 7) are streamed from L2, one M tile (b, t: k2 in [16 t, 16 t + 16))
//               ahead of the MFMAs, and reused across the N tiles.  The waves split the q1 ceil(r2 / 16) M tiles.  A lane's
//               accumulators are k2 = 16 t + 4 (l >> 4) .. + 3 of row (j, a) = l & 15: rounded to bf16 (nearest even) and written
//               as ONE 8-byte LDS store into X[j][a][b][k2].
//   product 2   row^T per lookup: M = c (Q2P / 16 tiles), N = 16 rows (a, b) of the lookup, K = k2.  A = the lookup's packed
//               core-2 slice [Q2P][K2p] (<= 8 x 16 bytes per lane, loaded once per lookup per wave), B = one ds_read_b128 per K
//               block from X.  The tiles (lookup, n-tile) are split over the waves.  A lane holds c = 4 (l >> 4) .. + 3 of row
//               (a, b) = l & 15: one 16-byte store to rows[lrec.x] (scalar stores where q2 % 4 != 0).
// X (bf16): row (j, a, b) at ((j q0 + a) AS + b S) bytes, S = 2 (K2p + 8) (S / 16 odd: the 16 rows of a product-2 read fall on 16
// different 16-byte bank groups), AS = q1 S (+ 16 where q1 is even: AS / 16 odd, so the 16 rows (j, a) of a product-1 store do
// too).  Columns [16 ceil(r2 / 16), K2p) are written by nobody else: zeroed once per work-group.  ONE X, two barriers per pass;
// the second work-group of the CU covers the other's barrier.
// Rows go out in ORIGINAL lookup order (lrec.x), each element written once: no atomics, bit-identical from run to run.
#include "ttx_internal.h"

namespace ttx {
namespace {

constexpr int kBmThreads = 256;
constexpr int kBmWaves = kBmThreads / kWave;
constexpr int kBmNT = 4;                // N tiles (16 rows (lookup, a)) of a pass, at most
constexpr int kBmRows = 16 * kBmNT;
constexpr int kBmMaxRank = 128;         // r1, r2
constexpr int kBmMaxQ2 = 32;
constexpr int kBmLdsGoal = 80 * 1024;   // LDS of a work-group that leaves room for two per CU
constexpr int kBmLdsMax = 160 * 1024;   // LDS of a work-group
constexpr int kBmRecBytes = 2 * 16 * kBmRows;  // two sets of lookup records (int4), used by alternate passes

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernels need of a geometry (host-derived; travels by value)
struct BmShape {
  int q0, q1, q2, r1, r2;
  int K1p, K2p;   // r1, r2 padded to the MFMA's K (32)
  int N1, N1p;    // q1 r2 columns of x_0, padded to 16 (the packed core 1)
  int Q2P;        // q2 padded to 16
  int MT;         // M tiles of a q1 block in product 1: ceil(r2 / 16)
  int R, NT2;     // rows (a, b) of a lookup, N tiles of a lookup in product 2
  int S, AS;      // bytes between rows b / between rows a of X
  int SC;         // lookups of a pass
  int D;
  int Sl[3];      // slices of core t
  int pe[3];      // packed bf16 elements of a slice of core t
  int lds_bytes;
};

// host-only: no Dims, no device.  false: not a shape of this kernel.
bool bm_shape(const ttx_geom* g, BmShape* o) {
  if (!g || g->T != 3 || g->num_tables <= 0 || g->r[0] != 1 || g->r[3] != 1) return false;
  for (int t = 0; t < 3; ++t)
    if (g->q[t] <= 0) return false;
  const int r1 = g->r[1], r2 = g->r[2];
  if (r1 <= 0 || r2 <= 0 || r1 > kBmMaxRank || r2 > kBmMaxRank) return false;
  if (g->q[0] > 16 || g->q[1] > 64 || g->q[2] > kBmMaxQ2) return false;
  BmShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.r1 = r1; s.r2 = r2;
  s.K1p = (r1 + 31) / 32 * 32;
  s.K2p = (r2 + 31) / 32 * 32;
  s.N1 = s.q1 * r2;
  s.N1p = (s.N1 + 15) / 16 * 16;
  s.Q2P = (s.q2 + 15) / 16 * 16;
  s.MT = (r2 + 15) / 16;
  s.R = s.q0 * s.q1;
  s.NT2 = (s.R + 15) / 16;
  s.S = 2 * (s.K2p + 8);                        // (K2p / 8 is a multiple of 4: S / 16 = K2p / 8 + 1 is odd)
  s.AS = s.q1 * s.S + (s.q1 % 2 == 0 ? 16 : 0);  // (q1 odd: q1 S / 16 is odd already)
  s.D = s.R * s.q2;
  s.pe[0] = s.q0 * s.K1p;
  s.pe[1] = s.N1p * s.K1p;
  s.pe[2] = s.Q2P * s.K2p;
  const int one = s.q0 * s.AS;  // X of one lookup
  if (one + kBmRecBytes > kBmLdsMax) return false;
  s.SC = kBmRows / s.q0;
  while (s.SC > 1 && s.SC * one + kBmRecBytes > kBmLdsGoal) --s.SC;
  s.lds_bytes = s.SC * one + kBmRecBytes;
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

// cores 0 and 1: the packed layout of ttx_tt_bf16.hip; core 2: [Q2P][K2p], row c, its k2 index contiguous (include/ttx.h)
__global__ __launch_bounds__(256) void pack_bf16m_kernel(int t, int pe, BmShape sh, long long total, const float* __restrict__ src,
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
    } else {              // [Q2P][K2p]: column c of the slice [r2][q2], its K index contiguous
      const int c = w / sh.K2p, k2 = w - c * sh.K2p;
      if (c < sh.q2 && k2 < sh.r2) at = sl * (sh.r2 * sh.q2) + k2 * sh.q2 + c;
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

// the A fragments of product 1's M tile mt = b MT + t: column k2 = 16 t + (l & 15) of q1 block b, k = 8 (l >> 4) .. + 7 of every
// 32; zero where the tile or the column does not exist (nothing is read there)
template <int KB>
__device__ __forceinline__ void load_a1(uint4 (&af)[KB], const unsigned short* __restrict__ base1, int mt, int nm, const BmShape& sh,
                                        int li, int lg) {
  const int b = mt / sh.MT;
  const int k2 = 16 * (mt - b * sh.MT) + li;
  const bool ok = mt < nm && k2 < sh.r2;
  const unsigned short* ap = base1 + (size_t)(ok ? b * sh.r2 + k2 : 0) * (KB * 32) + 8 * lg;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) af[kb] = ok ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
}

template <int KB, int K2B, int MQ>  // KB = K1p / 32, K2B = K2p / 32, MQ = Q2P / 16
__global__ __launch_bounds__(kBmThreads) void tt_rows_bf16m_kernel(const int4* __restrict__ chunk_rec, const int4* __restrict__ lrec,
                                                                   int nnz, BmShape sh, const unsigned short* __restrict__ c0,
                                                                   const unsigned short* __restrict__ c1,
                                                                   const unsigned short* __restrict__ c2, float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int4* Irec = (int4*)smem;                  // [2][64] records of a pass: {lookup n, slice of core 0, slice of core 2, -}
  unsigned char* X = smem + kBmRecBytes;     // [SC q0] row groups of AS bytes: x_0 of the pass, bf16
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
  const int nm = sh.q1 * sh.MT;  // M tiles of product 1
  // the columns product 1 never writes: 16 bf16 at [16 MT, K2p) of every row (a stale NaN there times core 2's zero padding is a
  // NaN); visible after the first barrier below
  if (16 * sh.MT < K2p) {
    const int nrow = sh.SC * sh.R;
    for (int e = tid; e < 2 * nrow; e += kBmThreads) {
      const int row = e >> 1;
      const int ja = row / sh.q1;
      *(uint4*)(X + (size_t)ja * sh.AS + (row - ja * sh.q1) * sh.S + 32 * sh.MT + 16 * (e & 1)) = make_uint4(0, 0, 0, 0);
    }
  }
  int4* I = Irec;
  for (int j0 = 0; j0 < len; j0 += sh.SC) {
    const int lenS = min(sh.SC, len - j0);
    const int rowsS = lenS * sh.q0;
    I = I == Irec ? Irec + kBmRows : Irec;  // (a wave still in the last pass's product 2 reads the other set)
    if (tid < lenS) {
      int4 r = lrec[start + j0 + tid];
      r.x = clampi(r.x, 0, nnz - 1);
      r.y = clampi(r.y, 0, sh.Sl[0] - 1);
      r.z = clampi(r.z, 0, sh.Sl[2] - 1);
      I[tid] = r;
    }
    __syncthreads();  // the records are there; every wave has left the last pass: its X is read
    // ---- product 1: the B fragments of the pass (row (j, a) = 16 nt + (l & 15), k = 8 (l >> 4) .. + 7), then the M tiles
    {
      uint4 bf[kBmNT][KB];
#pragma unroll
      for (int nt = 0; nt < kBmNT; ++nt) {
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
      for (int mt = wave; mt < nm; mt += kBmWaves) {
        uint4 an[KB];
        load_a1<KB>(an, base1, mt + kBmWaves, nm, sh, li, lg);  // (travels beside this tile's MFMAs)
        const int b = mt / sh.MT;
        unsigned char* xcol = X + b * sh.S + 2 * (16 * (mt - b * sh.MT) + 4 * lg);  // (16 t + 4 lg + 3 < 16 MT <= K2p)
#pragma unroll
        for (int nt = 0; nt < kBmNT; ++nt) {
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
    __syncthreads();  // X of the pass is whole
    // ---- product 2: tiles (lookup j, 16 rows (a, b)) over the waves; the lookup's core-2 fragments reloaded when j changes
    {
      uint4 cf[MQ][K2B];
      int jc = -1;
      const int ntile = lenS * sh.NT2;
      for (int tix = wave; tix < ntile; tix += kBmWaves) {
        const int j = tix / sh.NT2;
        const int4 rec = I[j];
        if (j != jc) {  // (wave-uniform) row c = 16 mq + (l & 15) of the slice, k2 = 8 (l >> 4) .. + 7 of every 32
          jc = j;
          const unsigned short* cp = c2 + (size_t)rec.z * sh.pe[2] + li * K2p + 8 * lg;
#pragma unroll
          for (int mq = 0; mq < MQ; ++mq)
#pragma unroll
            for (int kb = 0; kb < K2B; ++kb) cf[mq][kb] = *(const uint4*)(cp + mq * 16 * K2p + kb * 32);
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
            acc[mq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, cf[mq][kb]), __builtin_bit_cast(bf16x8, xv),
                                                              acc[mq], 0, 0, 0);
        }
        if (rho < sh.R) {
          float* out = rows + (size_t)rec.x * sh.D + (size_t)rho * sh.q2 + 4 * lg;
#pragma unroll
          for (int mq = 0; mq < MQ; ++mq) {
            const int c = 16 * mq + 4 * lg;
            if ((sh.q2 & 3) == 0) {  // (D % 4 == 0 and rows 16-byte aligned: the piece is too; c < q2 then c + 3 < q2)
              if (c < sh.q2) *(float4*)(out + 16 * mq) = make_float4(acc[mq][0], acc[mq][1], acc[mq][2], acc[mq][3]);
            } else {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                if (c + i < sh.q2) out[16 * mq + i] = acc[mq][i];
            }
          }
        }
      }
    }
    // (the next pass's first barrier stands between these reads of X and its stores)
  }
}

template <int KB, int K2B, int MQ>
int launch_rows(const Plan& P, int nnz, const BmShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  const void* fn = (const void*)tt_rows_bf16m_kernel<KB, K2B, MQ>;
  if (sh.lds_bytes > 48 * 1024) {
    const int rc = allow_dynamic_lds(fn, sh.lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tt_rows_bf16m_kernel<KB, K2B, MQ>), dim3(P.max_chunks), dim3(kBmThreads), sh.lds_bytes, st,
                     (const int4*)P.chunk_rec, (const int4*)P.lrec, nnz, sh, pc[0], pc[1], pc[2], rows);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

template <int KB, int K2B>
int launch_rows_mq(const Plan& P, int nnz, const BmShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  return sh.Q2P == 16 ? launch_rows<KB, K2B, 1>(P, nnz, sh, pc, rows, st) : launch_rows<KB, K2B, 2>(P, nnz, sh, pc, rows, st);
}

template <int KB>
int launch_rows_kb(const Plan& P, int nnz, const BmShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  switch (sh.K2p / 32) {
    case 1: return launch_rows_mq<KB, 1>(P, nnz, sh, pc, rows, st);
    case 2: return launch_rows_mq<KB, 2>(P, nnz, sh, pc, rows, st);
    case 3: return launch_rows_mq<KB, 3>(P, nnz, sh, pc, rows, st);
    default: return launch_rows_mq<KB, 4>(P, nnz, sh, pc, rows, st);
  }
}

}  // namespace
}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_rows_bf16m_supported(const ttx_geom* g) { return bm_shape(g, nullptr) ? 1 : 0; }

int64_t ttx_tt_pack_bf16m_elems(const ttx_geom* g, int32_t t) {
  BmShape sh;
  if (!bm_shape(g, &sh) || t < 0 || t > 2) return 0;
  long long S = 0;
  if (g->p_tables && g->num_tables > 1) {
    for (int k = 0; k < g->num_tables; ++k) {
      const int pk = g->p_tables[(size_t)k * 3 + t];
      if (pk <= 0) return 0;
      S += pk;
    }
  } else {
    if (g->p[t] <= 0) return 0;
    S = (long long)g->num_tables * g->p[t];
  }
  return S * sh.pe[t];
}

int ttx_tt_pack_bf16m(const ttx_geom* g, int32_t t, const float* core_f32, void* packed, ttx_stream_t stream) {
  BmShape sh;
  if (!g) TTX_FAIL(TTX_EINVAL, "pack_bf16m: geometry is NULL");
  if (!bm_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED, "pack_bf16m: not a shape of the MFMA-tail bf16 kernel (T = 3, ranks <= %d, q2 <= %d, x_0 of a lookup in LDS)",
             kBmMaxRank, kBmMaxQ2);
  if (t < 0 || t > 2) TTX_FAIL(TTX_EINVAL, "pack_bf16m: core %d out of range", t);
  const long long total = ttx_tt_pack_bf16m_elems(g, t);
  if (total <= 0) TTX_FAIL(TTX_EINVAL, "pack_bf16m: p must be > 0");
  if (!core_f32 || !packed) TTX_FAIL(TTX_EINVAL, "pack_bf16m: NULL input / output");
  if ((((uintptr_t)core_f32) & 3) || (((uintptr_t)packed) & 15))
    TTX_FAIL(TTX_EINVAL, "pack_bf16m: core_f32 must be 4-byte, packed 16-byte aligned");
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(pack_bf16m_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (int)t,
                     sh.pe[t], sh, total, core_f32, (unsigned short*)packed);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

size_t ttx_tt_rows_bf16m_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz) {
  (void)D;
  Dims d;
  if (!bm_shape(g, nullptr) || nnz < 0 || make_dims(g, &d) != TTX_OK) return 0;
  return plan_bytes(d, nnz) + 256;
}

int ttx_tt_rows_bf16m(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                      const void* const* packed_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                      ttx_stream_t stream) {
  Dims d;
  int rc = make_dims(g, &d);
  if (rc) return rc;
  BmShape sh;
  if (!bm_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED,
             "tt_rows_bf16m: not a shape of the MFMA-tail bf16 kernel (T = 3, ranks <= %d, q0 <= 16, q1 <= 64, q2 <= %d, x_0 of a lookup in LDS)",
             kBmMaxRank, kBmMaxQ2);
  if (D != d.D) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16m: D=%d does not match prod(q)=%d", D, d.D);
  if (nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16m: nnz=%lld out of range", (long long)nnz);
  if (nnz == 0) return TTX_OK;
  if (!packed_cores || !packed_cores[0] || !packed_cores[1] || !packed_cores[2] || !rows)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16m: NULL packed cores / rows");
  if ((((uintptr_t)packed_cores[0]) | ((uintptr_t)packed_cores[1]) | ((uintptr_t)packed_cores[2]) | ((uintptr_t)rows)) & 15)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16m: packed cores and rows must be 16-byte aligned");
  if (!plan && !indices) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16m: NULL indices (and no plan)");
  if (choose_chunk(d, nnz) <= 0) TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16m: no lookup plan for this shape");
  for (int t = 0; t < 3; ++t) sh.Sl[t] = d.S[t];
  hipStream_t st = (hipStream_t)stream;
  Plan P;
  if (plan) {
    P = carve_plan(d, nnz, (void*)plan);
  } else {
    const size_t pb = plan_bytes(d, nnz);
    if (!workspace || workspace_bytes < pb) TTX_FAIL(TTX_EWORKSPACE, "tt_rows_bf16m: workspace too small: %zu < %zu", workspace_bytes, pb);
    P = carve_plan(d, nnz, workspace);
    rc = plan_build(d, nnz, indices, tableidx, nullptr, P, st);
    if (rc) return rc;
  }
  const unsigned short* pc[3] = {(const unsigned short*)packed_cores[0], (const unsigned short*)packed_cores[1],
                                 (const unsigned short*)packed_cores[2]};
  switch (sh.K1p / 32) {
    case 1: return launch_rows_kb<1>(P, (int)nnz, sh, pc, rows, st);
    case 2: return launch_rows_kb<2>(P, (int)nnz, sh, pc, rows, st);
    case 3: return launch_rows_kb<3>(P, (int)nnz, sh, pc, rows, st);
    default: return launch_rows_kb<4>(P, (int)nnz, sh, pc, rows, st);
  }
}

}  // extern "C"
