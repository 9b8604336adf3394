// ttx_tt_bf16.hip -- bf16 inference forward of a three-core TT table (not in the reference): the cores rounded ONCE to bf16
// (ttx_tt_pack_bf16), the rows of a batch contracted from them on the bf16 MFMA with fp32 accumulation (ttx_tt_rows_bf16), and a
// segmented bag sum over rows in lookup order (ttx_bag_sum_pool).  Contract, packed layout and numerics bound: include/ttx.h,
// "bf16 inference forward"; DESIGN.md section 4.19.
//
// A work-group takes one pivot chunk of the plan (chunk_rec: <= MC lookups of ONE core-1 slice) and walks it in passes of
// SC = RP / q0 lookups = at most RP = 64 rows (lookup, a) of x_0 (32 / 16 where 64 do not fit the LDS):
//   product 1   x_0[(j, a), (b, k2)] = sum_k1 core_0[i0(j)][a, k1] core_1[s][k1, (b, k2)]   mfma_f32_16x16x32_bf16, fp32 accumulators.
//               A fragments (core 0: the rows of the pass, gathered by slice id) and B fragments (core 1: K contiguous per output
//               column) are single 16-byte loads of the packed cores; a wave keeps the A fragments of the pass's four M tiles in
//               registers and walks the N tiles, the accumulators go to LDS (row stride = q1 mod 64, q1 block stride r2 + 1: the
//               stores and the tail's reads are conflict-free).
//   product 2   row[j][a, b, c] = sum_k2 x_0[(j, a), (b, k2)] core_2[i2(j)][k2, c]   on the VALU from the fp32 x_0 (x_0 is NOT
//               rounded): one thread per (j, a, b), the q2 outputs in registers, core 2's [k2][Q2P] bf16 row one 8 / 16-byte load
//               -- from LDS where the pass's core-2 slices fit beside the tile with room for four work-groups per CU (STAGE: they
//               are requested behind the A fragments and carried across product 1 in registers, their latency beside the MFMAs;
//               327,680 lookups: 104.9 -> 93.9 us), from memory otherwise (ranks 64: staging would halve the pass and loses).
// Rows go out in ORIGINAL lookup order (lrec.x), each element written once: no atomics, bit-identical from run to run.
#include "ttx_internal.h"

namespace ttx {

constexpr int kBfThreads = 256;
constexpr int kBfWaves = kBfThreads / kWave;
constexpr int kBfMT = 4;                 // M tiles (16 rows) of a pass, at most
constexpr int kBfRows = 16 * kBfMT;      // rows (lookup, a) of a pass, at most
constexpr int kBfC2Regs = 4;             // 8-byte pieces of the pass's core-2 slices a thread carries to LDS
constexpr int kBfC2Bytes = kBfC2Regs * 8 * kBfThreads;  // ... = the core-2 bytes of a pass, at most
constexpr int kBfLdsGoal = 40 * 1024;    // LDS of a work-group that leaves room for four per CU
constexpr int kBfMaxRank = 64;           // r1, r2
constexpr int kBfMaxQ2 = 8;
constexpr int kBfLdsMax = 128 * 1024;    // LDS of a work-group

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernels need of a geometry (host-derived; travels by value)
struct BfShape {
  int q0, q1, q2, r1, r2;
  int K1p;        // r1 padded to the MFMA's K (32)
  int N1, N1p;    // q1 r2 columns of x_0, padded to 16
  int Q2P;        // q2 padded to 4 or 8
  int ld;         // floats between rows of x_0 in LDS
  int RP;         // rows of x_0 a pass may hold: 64, 32 or 16
  int SC;         // lookups of a pass
  int U2;         // 8-byte pieces of a packed core-2 slice
  int stage;      // the pass's core-2 slices go through LDS (they fit beside a 64-row tile); 0: the tail reads them from memory
  int D;
  int S[3];       // slices of core t
  int pe[3];      // packed bf16 elements of a slice of core t
  int lds_bytes;
};

// host-only: no Dims, no device.  false: not a shape of the bf16 kernel.
static bool bf_shape(const ttx_geom* g, BfShape* o) {
  if (!g || g->T != 3 || g->num_tables <= 0 || g->r[0] != 1 || g->r[3] != 1) return false;
  for (int t = 0; t < 3; ++t)
    if (g->q[t] <= 0) return false;
  const int r1 = g->r[1], r2 = g->r[2];
  if (r1 <= 0 || r2 <= 0 || r1 > kBfMaxRank || r2 > kBfMaxRank) return false;
  if (g->q[0] > 16 || g->q[1] > 64 || g->q[2] > kBfMaxQ2) return false;
  BfShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.r1 = r1; s.r2 = r2;
  s.K1p = (r1 + 31) / 32 * 32;
  s.N1 = s.q1 * r2;
  s.N1p = (s.N1 + 15) / 16 * 16;
  s.Q2P = s.q2 <= 4 ? 4 : 8;
  const int need = s.q1 * (r2 + 1);
  s.ld = need + ((s.q1 - need) % 64 + 64) % 64;  // smallest ld >= need with ld = q1 (mod 64)
  s.D = s.q0 * s.q1 * s.q2;
  s.pe[0] = s.q0 * s.K1p;
  s.pe[1] = s.N1p * s.K1p;
  s.pe[2] = r2 * s.Q2P;
  s.U2 = s.pe[2] / 4;
  // a pass of 64 rows with its lookups' core-2 slices staged in LDS, where that leaves room for four work-groups per CU ...
  s.RP = kBfRows;
  s.SC = s.RP / s.q0;
  s.lds_bytes = s.RP * s.ld * 4 + 16 * kBfRows + (s.SC * s.pe[2] * 2 + 15) / 16 * 16;  // x_0 tile, lookup records (int4), core-2 slices
  s.stage = (s.SC * s.pe[2] * 2 <= kBfC2Bytes && s.lds_bytes <= kBfLdsGoal) ? 1 : 0;
  if (!s.stage) {  // ... else the largest tile that fits at all; the tail reads core 2 from memory
    for (;; s.RP /= 2) {
      s.SC = s.RP / s.q0;
      s.lds_bytes = s.RP * s.ld * 4 + 16 * kBfRows;
      if (s.lds_bytes <= kBfLdsMax || s.RP == 16) break;
    }
  }
  if (s.lds_bytes > kBfLdsMax || s.SC < 1) return false;
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

__global__ __launch_bounds__(256) void pack_bf16_kernel(int t, int pe, BfShape sh, long long total,
                                                        const float* __restrict__ src, unsigned short* __restrict__ dst) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long sl = e / pe;  // (pe = sh.pe[t], as a scalar: no run-time subscript into the argument block)
    const int w = (int)(e - sl * pe);
    long long at = -1;  // the fp32 element, -1: padding
    if (t == 0) {        // [q0][K1p]
      const int a = w / sh.K1p, k = w - a * sh.K1p;
      if (k < sh.r1) at = sl * (sh.q0 * sh.r1) + a * sh.r1 + k;
    } else if (t == 1) {  // [N1p][K1p]: column n = b r2 + k2 of the slice [r1][q1][r2], its K index contiguous
      const int n = w / sh.K1p, k = w - n * sh.K1p;
      if (n < sh.N1 && k < sh.r1) at = sl * ((long long)sh.r1 * sh.N1) + (long long)k * sh.N1 + n;
    } else {              // [r2][Q2P]
      const int k2 = w / sh.Q2P, c = w - k2 * sh.Q2P;
      if (c < sh.q2) at = sl * (sh.r2 * sh.q2) + k2 * sh.q2 + c;
    }
    dst[e] = at >= 0 ? bf16_rne(src[at]) : (unsigned short)0;
  }
}

// ---------------------------------------------------------------- rows -----
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ float bf_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

template <int KB, int Q2P, bool STAGE>  // KB = K1p / 32; STAGE: BfShape::stage
__global__ __launch_bounds__(kBfThreads) void tt_rows_bf16_kernel(const int4* __restrict__ chunk_rec, const int4* __restrict__ lrec,
                                                                  int nnz, BfShape sh, const unsigned short* __restrict__ c0,
                                                                  const unsigned short* __restrict__ c1,
                                                                  const unsigned short* __restrict__ c2, float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* X0 = smem;                                // [RP][ld]
  int4* I = (int4*)(smem + sh.RP * sh.ld);         // [SC] records of the pass: {lookup n, slice of core 0, slice of core 2, -}
  uint2* C2s = (uint2*)(I + kBfRows);              // [SC][U2] the pass's core-2 slices, packed bf16
  const int4 cr = chunk_rec[blockIdx.x];
  if (cr.z <= 0) return;
  // (the plan is trusted for its order, not for memory safety: every index it hands over is clamped)
  const int s = clampi(cr.x, 0, sh.S[1] - 1);
  const int start = clampi(cr.y, 0, nnz);
  const int len = min(cr.z, nnz - start);
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int li = lane & 15, lg = lane >> 4;
  const int K1p = KB * 32;
  const unsigned short* base1 = c1 + (size_t)s * sh.pe[1];
  const int ntiles = sh.N1p / 16;
  const int q01 = sh.q0 * sh.q1;
  for (int j0 = 0; j0 < len; j0 += sh.SC) {
    const int lenS = min(sh.SC, len - j0);
    const int rowsS = lenS * sh.q0;
    if (tid < lenS) {
      int4 r = lrec[start + j0 + tid];
      r.x = clampi(r.x, 0, nnz - 1);
      r.y = clampi(r.y, 0, sh.S[0] - 1);
      r.z = clampi(r.z, 0, sh.S[2] - 1);
      I[tid] = r;
    }
    __syncthreads();
    // ---- product 1: the A fragments of the pass's M tiles (row m = (j, a) on lanes l & 15, k = 8 (l >> 4) .. + 7)
    uint4 af[kBfMT][KB];
#pragma unroll
    for (int mt = 0; mt < kBfMT; ++mt) {
      const int m = mt * 16 + li;
      const bool live = m < rowsS;
      const int j = live ? m / sh.q0 : 0;
      const int a = live ? m - j * sh.q0 : 0;
      const unsigned short* ap = c0 + (size_t)I[j].y * sh.pe[0] + a * K1p + 8 * lg;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) af[mt][kb] = live ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
    }
    // the pass's core-2 slices: requested now, carried to LDS behind product 1 (their latency runs beside it)
    uint2 c2r[kBfC2Regs];
    const int c2n = STAGE ? lenS * sh.U2 : 0;  // (<= kBfC2Regs * kBfThreads: bf_shape)
    if constexpr (STAGE) {
#pragma unroll
      for (int u = 0; u < kBfC2Regs; ++u) {
        const int e = tid + u * kBfThreads;
        c2r[u] = make_uint2(0, 0);
        if (e < c2n) {
          const int j = e / sh.U2;
          c2r[u] = ((const uint2*)(c2 + (size_t)I[j].z * sh.pe[2]))[e - j * sh.U2];
        }
      }
    }
    for (int nt = wave; nt < ntiles; nt += kBfWaves) {
      const int n = nt * 16 + li;  // (< N1p: the packed slice holds zero columns up to it)
      const unsigned short* bp = base1 + (size_t)n * K1p + 8 * lg;
      uint4 bfr[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) bfr[kb] = *(const uint4*)(bp + kb * 32);
      const int b = n / sh.r2;
      const int xoff = b * (sh.r2 + 1) + (n - b * sh.r2);
#pragma unroll
      for (int mt = 0; mt < kBfMT; ++mt) {
        if (mt * 16 < rowsS) {  // (wave-uniform)
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; ++kb)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[mt][kb]), __builtin_bit_cast(bf16x8, bfr[kb]),
                                                          acc, 0, 0, 0);
          if (n < sh.N1) {  // C/D: column n on lanes l & 15, rows 4 (l >> 4) + i
            float* xp = X0 + (mt * 16 + 4 * lg) * sh.ld + xoff;
            xp[0] = acc[0];
            xp[sh.ld] = acc[1];
            xp[2 * sh.ld] = acc[2];
            xp[3 * sh.ld] = acc[3];
          }
        }
      }
    }
    if constexpr (STAGE) {
#pragma unroll
      for (int u = 0; u < kBfC2Regs; ++u) {
        const int e = tid + u * kBfThreads;
        if (e < c2n) C2s[e] = c2r[u];
      }
    }
    __syncthreads();
    // ---- product 2: one thread per (j, a, b), fp32 x_0 from LDS, the lookup's packed core-2 slice from LDS (STAGE) or memory
    const int items = rowsS * sh.q1;
    for (int it = tid; it < items; it += kBfThreads) {
      const int m = it / sh.q1, b = it - m * sh.q1;
      const int j = m / sh.q0;
      const int4 rec = I[j];
      const uint2* cp = STAGE ? C2s + j * sh.U2 : (const uint2*)(c2 + (size_t)rec.z * sh.pe[2]);
      const float* x = X0 + m * sh.ld + b * (sh.r2 + 1);
      float o[Q2P];
#pragma unroll
      for (int c = 0; c < Q2P; ++c) o[c] = 0.f;
#pragma unroll 4
      for (int k2 = 0; k2 < sh.r2; ++k2) {
        const float xv = x[k2];
        if constexpr (Q2P == 4) {
          const uint2 w = cp[k2];
          o[0] = fmaf(xv, bf_lo(w.x), o[0]); o[1] = fmaf(xv, bf_hi(w.x), o[1]);
          o[2] = fmaf(xv, bf_lo(w.y), o[2]); o[3] = fmaf(xv, bf_hi(w.y), o[3]);
        } else {
          const uint4 w = *(const uint4*)(cp + 2 * k2);
          o[0] = fmaf(xv, bf_lo(w.x), o[0]); o[1] = fmaf(xv, bf_hi(w.x), o[1]);
          o[2] = fmaf(xv, bf_lo(w.y), o[2]); o[3] = fmaf(xv, bf_hi(w.y), o[3]);
          o[4] = fmaf(xv, bf_lo(w.z), o[4]); o[5] = fmaf(xv, bf_hi(w.z), o[5]);
          o[6] = fmaf(xv, bf_lo(w.w), o[6]); o[7] = fmaf(xv, bf_hi(w.w), o[7]);
        }
      }
      float* out = rows + (size_t)rec.x * sh.D + (size_t)(it - j * q01) * sh.q2;
      if (sh.q2 == Q2P) {  // (D % 4 == 0 and rows 16-byte aligned: the piece is too)
        *(float4*)out = make_float4(o[0], o[1], o[2], o[3]);
        if constexpr (Q2P == 8) *(float4*)(out + 4) = make_float4(o[4], o[5], o[6], o[7]);
      } else {
#pragma unroll
        for (int c = 0; c < Q2P; ++c)
          if (c < sh.q2) out[c] = o[c];
      }
    }
    __syncthreads();  // the next pass rewrites I, X0 and C2s
  }
}

template <int KB, int Q2P, bool STAGE>
static int launch_rows(const Plan& P, int nnz, const BfShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  const void* fn = (const void*)tt_rows_bf16_kernel<KB, Q2P, STAGE>;
  if (sh.lds_bytes > 48 * 1024) {
    const int rc = allow_dynamic_lds(fn, sh.lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tt_rows_bf16_kernel<KB, Q2P, STAGE>), dim3(P.max_chunks), dim3(kBfThreads), sh.lds_bytes, st,
                     (const int4*)P.chunk_rec, (const int4*)P.lrec, nnz, sh, pc[0], pc[1], pc[2], rows);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

// ---------------------------------------------------------------- pool -----
// output[b, :] = rows[offsets[b]] + rows[offsets[b] + 1] + ... in index order, starting from +0: one thread per (bag, piece of
// the row), V = float4 (D % 4 == 0, both pointers 16-byte aligned) or float; consecutive lanes hold consecutive pieces.
__device__ __forceinline__ void acc_add(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ void acc_add(float& a, const float v) { a += v; }

template <typename V>
__global__ __launch_bounds__(256) void bag_sum_pool_kernel(long long nb, int DP, const int64_t* __restrict__ offsets,
                                                           const V* __restrict__ rows, V* __restrict__ out) {
  const long long total = nb * DP;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long bag = e / DP;
    const int c = (int)(e - bag * DP);
    long long a = offsets[bag], z = offsets[bag + 1];
    a = a < 0 ? 0 : a;
    V acc = V{};
    const V* p = rows + a * DP + c;
    long long j = a;
    for (; j + 3 < z; j += 4, p += 4 * (long long)DP) {  // four rows in flight, added in index order
      const V v0 = p[0], v1 = p[DP], v2 = p[2 * (long long)DP], v3 = p[3 * (long long)DP];
      acc_add(acc, v0); acc_add(acc, v1); acc_add(acc, v2); acc_add(acc, v3);
    }
    for (; j < z; ++j, p += DP) acc_add(acc, p[0]);
    out[e] = acc;
  }
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_rows_bf16_supported(const ttx_geom* g) { return bf_shape(g, nullptr) ? 1 : 0; }

int64_t ttx_tt_pack_bf16_elems(const ttx_geom* g, int32_t t) {
  BfShape sh;
  if (!bf_shape(g, &sh) || t < 0 || t > 2) return 0;
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

int ttx_tt_pack_bf16(const ttx_geom* g, int32_t t, const float* core_f32, void* packed, ttx_stream_t stream) {
  BfShape sh;
  if (!g) TTX_FAIL(TTX_EINVAL, "pack_bf16: geometry is NULL");
  if (!bf_shape(g, &sh)) TTX_FAIL(TTX_EUNSUPPORTED, "pack_bf16: not a shape of the bf16 kernel (T = 3, ranks <= %d, q2 <= %d)", kBfMaxRank, kBfMaxQ2);
  if (t < 0 || t > 2) TTX_FAIL(TTX_EINVAL, "pack_bf16: core %d out of range", t);
  const long long total = ttx_tt_pack_bf16_elems(g, t);
  if (total <= 0) TTX_FAIL(TTX_EINVAL, "pack_bf16: p must be > 0");
  if (!core_f32 || !packed) TTX_FAIL(TTX_EINVAL, "pack_bf16: NULL input / output");
  if ((((uintptr_t)core_f32) & 3) || (((uintptr_t)packed) & 15)) TTX_FAIL(TTX_EINVAL, "pack_bf16: core_f32 must be 4-byte, packed 16-byte aligned");
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(pack_bf16_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (int)t,
                     sh.pe[t], sh, total, core_f32, (unsigned short*)packed);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

size_t ttx_tt_rows_bf16_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz) {
  (void)D;
  Dims d;
  if (!bf_shape(g, nullptr) || nnz < 0 || make_dims(g, &d) != TTX_OK) return 0;
  return plan_bytes(d, nnz) + 256;
}

int ttx_tt_rows_bf16(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                     const void* const* packed_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                     ttx_stream_t stream) {
  Dims d;
  int rc = make_dims(g, &d);
  if (rc) return rc;
  BfShape sh;
  if (!bf_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16: not a shape of the bf16 kernel (T = 3, ranks <= %d, q2 <= %d, the x_0 tile within the LDS)",
             kBfMaxRank, kBfMaxQ2);
  if (D != d.D) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16: D=%d does not match prod(q)=%d", D, d.D);
  if (nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16: nnz=%lld out of range", (long long)nnz);
  if (nnz == 0) return TTX_OK;
  if (!packed_cores || !packed_cores[0] || !packed_cores[1] || !packed_cores[2] || !rows)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16: NULL packed cores / rows");
  if ((((uintptr_t)packed_cores[0]) | ((uintptr_t)packed_cores[1]) | ((uintptr_t)packed_cores[2]) | ((uintptr_t)rows)) & 15)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16: packed cores and rows must be 16-byte aligned");
  if (!plan && !indices) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16: NULL indices (and no plan)");
  if (choose_chunk(d, nnz) <= 0) TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16: no lookup plan for this shape");
  for (int t = 0; t < 3; ++t) sh.S[t] = d.S[t];
  hipStream_t st = (hipStream_t)stream;
  Plan P;
  if (plan) {
    P = carve_plan(d, nnz, (void*)plan);
  } else {
    const size_t pb = plan_bytes(d, nnz);
    if (!workspace || workspace_bytes < pb) TTX_FAIL(TTX_EWORKSPACE, "tt_rows_bf16: workspace too small: %zu < %zu", workspace_bytes, pb);
    P = carve_plan(d, nnz, workspace);
    rc = plan_build(d, nnz, indices, tableidx, nullptr, P, st);
    if (rc) return rc;
  }
  const unsigned short* pc[3] = {(const unsigned short*)packed_cores[0], (const unsigned short*)packed_cores[1],
                                 (const unsigned short*)packed_cores[2]};
#define TTX_BF_ROWS(KB, Q2P) \
  (sh.stage ? launch_rows<KB, Q2P, true>(P, (int)nnz, sh, pc, rows, st) : launch_rows<KB, Q2P, false>(P, (int)nnz, sh, pc, rows, st))
  if (sh.K1p == 32) return sh.Q2P == 4 ? TTX_BF_ROWS(1, 4) : TTX_BF_ROWS(1, 8);
  return sh.Q2P == 4 ? TTX_BF_ROWS(2, 4) : TTX_BF_ROWS(2, 8);
#undef TTX_BF_ROWS
}

int ttx_bag_sum_pool(int64_t nb, int32_t D, const int64_t* offsets, const float* rows, float* output, ttx_stream_t stream) {
  if (nb < 0 || D <= 0 || nb >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bag_sum_pool: bad nb / D (nb=%lld, D=%d)", (long long)nb, D);
  if (nb == 0) return TTX_OK;
  if (!offsets || !rows || !output) TTX_FAIL(TTX_EINVAL, "bag_sum_pool: NULL input / output");
  if ((((uintptr_t)rows) | ((uintptr_t)output)) & 3) TTX_FAIL(TTX_EINVAL, "bag_sum_pool: float pointers must be 4-byte aligned");
  if (((uintptr_t)offsets) & 7) TTX_FAIL(TTX_EINVAL, "bag_sum_pool: offsets must be 8-byte aligned");
  const bool v4 = D % 4 == 0 && ((((uintptr_t)rows) | ((uintptr_t)output)) & 15) == 0;
  const int DP = v4 ? D / 4 : D;
  const long long blocks = (nb * DP + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20));
  if (v4)
    hipLaunchKernelGGL(bag_sum_pool_kernel<float4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)nb, DP, offsets,
                       (const float4*)rows, (float4*)output);
  else
    hipLaunchKernelGGL(bag_sum_pool_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)nb, DP, offsets, rows,
                       output);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"
