// ttx_tt_bf16w.hip -- the COLUMN-BLOCKED bf16 inference forward of a three-core TT table: ranks up to 128 and any q1 <= 64, the
// shapes the narrow kernel (ttx_tt_bf16.hip) refuses because it holds a whole x_0 tile in LDS.  Same packed layout, same plan,
// same contract and numerics bound: include/ttx.h "bf16 inference forward, column-blocked"; DESIGN.md section 4.20.
//
// A work-group takes one pivot chunk of the plan (chunk_rec: <= MC lookups of ONE core-1 slice) and walks it in passes of
// SC = 64 / q0 lookups = at most 64 rows (lookup, a).  The A fragments of the pass (core 0: four M tiles x KB = K1p / 32 16-byte
// loads per lane, <= 64 VGPRs) stay in registers for the whole pass; x_0 is NEVER held whole.  The pass walks the q1 blocks b:
//   product 1   x_0[(j, a), (b, k2)] for ONE b: the four waves split the NT = ceil(r2 / 16) N tiles (k2 in [16 t, 16 t + 16)), KB
//               mfma_f32_16x16x32_bf16 per M tile, fp32 accumulators stored to an LDS tile [64][ldt] (ldt >= 16 NT, ldt / 4 odd:
//               the accumulator stores and the tail's 16-byte reads are conflict-free).  Columns with k2 >= r2 are not loaded
//               (r2 need not be a multiple of 16, a block need not start on a 16-column boundary of the packed slice): their B
//               fragment is zero and so is their x_0.
//   product 2   row[j][a, b, :] = sum_k2 x_0[(j, a), (b, k2)] core_2[i2(j)][k2, :] on the VALU from the fp32 x_0 (NOT rounded).
//               A block has only 64 items (j, a): each item runs on FOUR adjacent lanes, lane h of the quad taking
//               k2 = 16 g + 4 h .. + 3 of every group g of 16 (one 16-byte LDS read), Q2P partial sums in registers, combined
//               across the quad by two DPP quad_perm adds in a fixed order; lane 0 of the quad stores the q2 floats.
// TWO tiles, used alternately: iteration b runs the MFMAs of block b + 1 into one tile, requests the B fragments of block b + 2
// (their latency runs beside the tail) and reads block b's tile in the tail -- ONE barrier per block.  The pass's core-2 slices
// are staged in LDS (STAGE) where tiles + records + slices stay within 80 KiB (two work-groups per CU), else read from memory.
// Rows go out in ORIGINAL lookup order (lrec.x), each element written once: no atomics, bit-identical from run to run.
#include "ttx_internal.h"

namespace ttx {
namespace {

constexpr int kBwThreads = 256;
constexpr int kBwWaves = kBwThreads / kWave;
constexpr int kBwMT = 4;                // M tiles (16 rows) of a pass
constexpr int kBwRows = 16 * kBwMT;     // rows (lookup, a) of a pass
constexpr int kBwMaxRank = 128;         // r1, r2
constexpr int kBwMaxQ2 = 8;
constexpr int kBwNTW = kBwMaxRank / 16 / kBwWaves;  // N tiles of a block a wave takes, at most (2)
constexpr int kBwLdsGoal = 80 * 1024;   // LDS of a work-group that leaves room for two per CU

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernels need of a geometry (host-derived; travels by value)
struct BwShape {
  int q0, q1, q2, r1, r2;
  int K1p;        // r1 padded to the MFMA's K (32)
  int N1, N1p;    // q1 r2 columns of x_0, padded to 16 (the packed core 1)
  int Q2P;        // q2 padded to 4 or 8
  int NT;         // N tiles of a q1 block
  int ldt;        // floats between rows of an LDS tile
  int SC;         // lookups of a pass
  int U2;         // 8-byte pieces of a packed core-2 slice
  int stage;      // the pass's core-2 slices go through LDS
  int D;
  int S[3];       // slices of core t
  int pe[3];      // packed bf16 elements of a slice of core t
  int lds_bytes;
};

// host-only: no Dims, no device.  false: not a shape of the column-blocked kernel.
bool bw_shape(const ttx_geom* g, BwShape* o) {
  if (!g || g->T != 3 || g->num_tables <= 0 || g->r[0] != 1 || g->r[3] != 1) return false;
  for (int t = 0; t < 3; ++t)
    if (g->q[t] <= 0) return false;
  const int r1 = g->r[1], r2 = g->r[2];
  if (r1 <= 0 || r2 <= 0 || r1 > kBwMaxRank || r2 > kBwMaxRank) return false;
  if (g->q[0] > 16 || g->q[1] > 64 || g->q[2] > kBwMaxQ2) return false;
  BwShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.r1 = r1; s.r2 = r2;
  s.K1p = (r1 + 31) / 32 * 32;
  s.N1 = s.q1 * r2;
  s.N1p = (s.N1 + 15) / 16 * 16;
  s.Q2P = s.q2 <= 4 ? 4 : 8;
  s.NT = (r2 + 15) / 16;
  s.ldt = 16 * s.NT + 4;  // (16 NT is a multiple of 8: ldt / 4 is odd)
  s.D = s.q0 * s.q1 * s.q2;
  s.pe[0] = s.q0 * s.K1p;
  s.pe[1] = s.N1p * s.K1p;
  s.pe[2] = r2 * s.Q2P;
  s.U2 = s.pe[2] / 4;
  s.SC = kBwRows / s.q0;
  const int base = 2 * kBwRows * s.ldt * 4 + 16 * kBwRows;  // two tiles, lookup records (int4): <= 67 KiB + 1 KiB at r2 = 128
  const int c2 = (s.SC * s.pe[2] * 2 + 15) / 16 * 16;
  s.stage = base + c2 <= kBwLdsGoal ? 1 : 0;
  s.lds_bytes = base + (s.stage ? c2 : 0);
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

// the packed layout of ttx_tt_bf16.hip (include/ttx.h), for any rank of this kernel's domain
__global__ __launch_bounds__(256) void pack_bf16w_kernel(int t, int pe, BwShape sh, long long total, const float* __restrict__ src,
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

// v + (v of the lane the quad permutation CTRL names): 0xB1 = [1, 0, 3, 2], 0x4E = [2, 3, 0, 1]
template <int CTRL>
__device__ __forceinline__ float quad_add(float v) {
  const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, true);
  return v + __int_as_float(o);
}

// the B fragments of q1 block b for this wave's N tiles t = wave, wave + 4: column k2 = 16 t + (l & 15), k = 8 (l >> 4) .. + 7 of
// every 32; zero where the block, the tile or the column does not exist (nothing is read there)
template <int KB>
__device__ __forceinline__ void load_b(uint4 (&bf)[kBwNTW][KB], const unsigned short* __restrict__ base1, int b, const BwShape& sh,
                                       int wave, int li, int lg) {
#pragma unroll
  for (int u = 0; u < kBwNTW; ++u) {
    const int k2 = 16 * (wave + kBwWaves * u) + li;
    const bool ok = b < sh.q1 && k2 < sh.r2;
    const unsigned short* bp = base1 + (size_t)(ok ? b * sh.r2 + k2 : 0) * (KB * 32) + 8 * lg;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) bf[u][kb] = ok ? *(const uint4*)(bp + kb * 32) : make_uint4(0, 0, 0, 0);
  }
}

// x_0 of one q1 block from the fragments -> tile [64][ldt] (C/D: column on lanes l & 15, rows 4 (l >> 4) + i)
template <int KB>
__device__ __forceinline__ void mma_store(const uint4 (&af)[kBwMT][KB], const uint4 (&bf)[kBwNTW][KB], float* __restrict__ tile,
                                          const BwShape& sh, int rowsS, int wave, int li, int lg) {
#pragma unroll
  for (int u = 0; u < kBwNTW; ++u) {
    const int t = wave + kBwWaves * u;
    if (t < sh.NT) {  // (wave-uniform)
#pragma unroll
      for (int mt = 0; mt < kBwMT; ++mt) {
        if (mt * 16 < rowsS) {  // (wave-uniform)
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int kb = 0; kb < KB; ++kb)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[mt][kb]), __builtin_bit_cast(bf16x8, bf[u][kb]),
                                                          acc, 0, 0, 0);
          float* xp = tile + (mt * 16 + 4 * lg) * sh.ldt + 16 * t + li;  // (16 t + li < 16 NT < ldt)
          xp[0] = acc[0];
          xp[sh.ldt] = acc[1];
          xp[2 * sh.ldt] = acc[2];
          xp[3 * sh.ldt] = acc[3];
        }
      }
    }
  }
}

template <int KB, int Q2P, bool STAGE>  // KB = K1p / 32; STAGE: BwShape::stage
__global__ __launch_bounds__(kBwThreads) void tt_rows_bf16w_kernel(const int4* __restrict__ chunk_rec, const int4* __restrict__ lrec,
                                                                   int nnz, BwShape sh, const unsigned short* __restrict__ c0,
                                                                   const unsigned short* __restrict__ c1,
                                                                   const unsigned short* __restrict__ c2, float* __restrict__ rows) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* T0 = smem;                                 // [64][ldt] x_0 of the even q1 blocks
  float* T1 = smem + kBwRows * sh.ldt;              // ... of the odd ones
  int4* I = (int4*)(smem + 2 * kBwRows * sh.ldt);   // [SC] records of the pass: {lookup n, slice of core 0, slice of core 2, -}
  uint2* C2s = (uint2*)(I + kBwRows);               // [SC][U2] the pass's core-2 slices, packed bf16 (STAGE)
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
  const int tm = tid >> 2, th = tid & 3;  // the tail's item (row of the pass) and this lane's quarter of k2
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
    // ---- the A fragments of the pass's M tiles (row m = (j, a) on lanes l & 15, k = 8 (l >> 4) .. + 7), the B fragments of block 0
    uint4 af[kBwMT][KB];
#pragma unroll
    for (int mt = 0; mt < kBwMT; ++mt) {
      const int m = mt * 16 + li;
      const bool live = m < rowsS;
      const int j = live ? m / sh.q0 : 0;
      const int a = live ? m - j * sh.q0 : 0;
      const unsigned short* ap = c0 + (size_t)I[j].y * sh.pe[0] + a * K1p + 8 * lg;
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) af[mt][kb] = live ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
    }
    uint4 bf[kBwNTW][KB];
    load_b<KB>(bf, base1, 0, sh, wave, li, lg);
    // the pass's core-2 slices, requested behind the fragments (visible to the tail after the barrier below)
    if constexpr (STAGE) {
      const int c2n = lenS * sh.U2;
      for (int e = tid; e < c2n; e += kBwThreads) {
        const int j = e / sh.U2;
        C2s[e] = ((const uint2*)(c2 + (size_t)I[j].z * sh.pe[2]))[e - j * sh.U2];
      }
    }
    // the tail's item: its lookup, its core-2 slice, where its row piece goes
    const bool tlive = tm < rowsS;
    const int tj = tlive ? tm / sh.q0 : 0;
    const int4 rec = I[tj];
    const uint2* cp = STAGE ? C2s + tj * sh.U2 : (const uint2*)(c2 + (size_t)rec.z * sh.pe[2]);
    const float* xrow = T0 + tm * sh.ldt + 4 * th;
    float* orow = rows + (size_t)rec.x * sh.D + (size_t)(tm - tj * sh.q0) * sh.q1 * sh.q2;
    mma_store<KB>(af, bf, T0, sh, rowsS, wave, li, lg);
    load_b<KB>(bf, base1, 1, sh, wave, li, lg);
    __syncthreads();
    for (int b = 0; b < sh.q1; ++b) {
      const int odd = b & 1;
      // ---- product 1 of block b + 1 into the other tile; the fragments of block b + 2 travel beside the tail
      if (b + 1 < sh.q1) {
        mma_store<KB>(af, bf, odd ? T0 : T1, sh, rowsS, wave, li, lg);
        load_b<KB>(bf, base1, b + 2, sh, wave, li, lg);
      }
      // ---- product 2 of block b: this lane's quarter of k2, then the quad's sum
      float o[Q2P];
#pragma unroll
      for (int c = 0; c < Q2P; ++c) o[c] = 0.f;
      if (tlive) {
        const float* x = xrow + (odd ? kBwRows * sh.ldt : 0);
        for (int g = 0; g < sh.NT; ++g) {
          const float4 xv4 = *(const float4*)(x + 16 * g);
          const float xs[4] = {xv4.x, xv4.y, xv4.z, xv4.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int k2 = 16 * g + 4 * th + i;
            if (k2 < sh.r2) {
              const float xv = xs[i];
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
          }
        }
      }
#pragma unroll
      for (int c = 0; c < Q2P; ++c) o[c] = quad_add<0x4E>(quad_add<0xB1>(o[c]));  // (h0 + h1) + (h2 + h3)
      if (tlive && th == 0) {
        float* out = orow + b * sh.q2;
        if (sh.q2 == Q2P) {  // (D % 4 == 0 and rows 16-byte aligned: the piece is too)
          *(float4*)out = make_float4(o[0], o[1], o[2], o[3]);
          if constexpr (Q2P == 8) *(float4*)(out + 4) = make_float4(o[4], o[5], o[6], o[7]);
        } else {
#pragma unroll
          for (int c = 0; c < Q2P; ++c)
            if (c < sh.q2) out[c] = o[c];
        }
      }
      __syncthreads();  // block b + 1's tile is whole, block b's tile is read; after the last block: the next pass rewrites I, C2s
    }
  }
}

template <int KB, int Q2P, bool STAGE>
int launch_rows(const Plan& P, int nnz, const BwShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  const void* fn = (const void*)tt_rows_bf16w_kernel<KB, Q2P, STAGE>;
  if (sh.lds_bytes > 48 * 1024) {
    const int rc = allow_dynamic_lds(fn, sh.lds_bytes);
    if (rc) return rc;
  }
  hipLaunchKernelGGL((tt_rows_bf16w_kernel<KB, Q2P, STAGE>), dim3(P.max_chunks), dim3(kBwThreads), sh.lds_bytes, st,
                     (const int4*)P.chunk_rec, (const int4*)P.lrec, nnz, sh, pc[0], pc[1], pc[2], rows);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

template <int KB>
int launch_rows_kb(const Plan& P, int nnz, const BwShape& sh, const unsigned short* const* pc, float* rows, hipStream_t st) {
  if (sh.Q2P == 4)
    return sh.stage ? launch_rows<KB, 4, true>(P, nnz, sh, pc, rows, st) : launch_rows<KB, 4, false>(P, nnz, sh, pc, rows, st);
  return sh.stage ? launch_rows<KB, 8, true>(P, nnz, sh, pc, rows, st) : launch_rows<KB, 8, false>(P, nnz, sh, pc, rows, st);
}

}  // namespace
}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_rows_bf16w_supported(const ttx_geom* g) { return bw_shape(g, nullptr) ? 1 : 0; }

int64_t ttx_tt_pack_bf16w_elems(const ttx_geom* g, int32_t t) {
  BwShape sh;
  if (!bw_shape(g, &sh) || t < 0 || t > 2) return 0;
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

int ttx_tt_pack_bf16w(const ttx_geom* g, int32_t t, const float* core_f32, void* packed, ttx_stream_t stream) {
  BwShape sh;
  if (!g) TTX_FAIL(TTX_EINVAL, "pack_bf16w: geometry is NULL");
  if (!bw_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED, "pack_bf16w: not a shape of the column-blocked bf16 kernel (T = 3, ranks <= %d, q2 <= %d)", kBwMaxRank,
             kBwMaxQ2);
  if (t < 0 || t > 2) TTX_FAIL(TTX_EINVAL, "pack_bf16w: core %d out of range", t);
  const long long total = ttx_tt_pack_bf16w_elems(g, t);
  if (total <= 0) TTX_FAIL(TTX_EINVAL, "pack_bf16w: p must be > 0");
  if (!core_f32 || !packed) TTX_FAIL(TTX_EINVAL, "pack_bf16w: NULL input / output");
  if ((((uintptr_t)core_f32) & 3) || (((uintptr_t)packed) & 15))
    TTX_FAIL(TTX_EINVAL, "pack_bf16w: core_f32 must be 4-byte, packed 16-byte aligned");
  const long long blocks = (total + 255) / 256;
  hipLaunchKernelGGL(pack_bf16w_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, (int)t,
                     sh.pe[t], sh, total, core_f32, (unsigned short*)packed);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

size_t ttx_tt_rows_bf16w_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz) {
  (void)D;
  Dims d;
  if (!bw_shape(g, nullptr) || nnz < 0 || make_dims(g, &d) != TTX_OK) return 0;
  return plan_bytes(d, nnz) + 256;
}

int ttx_tt_rows_bf16w(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                      const void* const* packed_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                      ttx_stream_t stream) {
  Dims d;
  int rc = make_dims(g, &d);
  if (rc) return rc;
  BwShape sh;
  if (!bw_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16w: not a shape of the column-blocked bf16 kernel (T = 3, ranks <= %d, q0 <= 16, q1 <= 64, q2 <= %d)",
             kBwMaxRank, kBwMaxQ2);
  if (D != d.D) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16w: D=%d does not match prod(q)=%d", D, d.D);
  if (nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16w: nnz=%lld out of range", (long long)nnz);
  if (nnz == 0) return TTX_OK;
  if (!packed_cores || !packed_cores[0] || !packed_cores[1] || !packed_cores[2] || !rows)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16w: NULL packed cores / rows");
  if ((((uintptr_t)packed_cores[0]) | ((uintptr_t)packed_cores[1]) | ((uintptr_t)packed_cores[2]) | ((uintptr_t)rows)) & 15)
    TTX_FAIL(TTX_EINVAL, "tt_rows_bf16w: packed cores and rows must be 16-byte aligned");
  if (!plan && !indices) TTX_FAIL(TTX_EINVAL, "tt_rows_bf16w: NULL indices (and no plan)");
  if (choose_chunk(d, nnz) <= 0) TTX_FAIL(TTX_EUNSUPPORTED, "tt_rows_bf16w: no lookup plan for this shape");
  for (int t = 0; t < 3; ++t) sh.S[t] = d.S[t];
  hipStream_t st = (hipStream_t)stream;
  Plan P;
  if (plan) {
    P = carve_plan(d, nnz, (void*)plan);
  } else {
    const size_t pb = plan_bytes(d, nnz);
    if (!workspace || workspace_bytes < pb) TTX_FAIL(TTX_EWORKSPACE, "tt_rows_bf16w: workspace too small: %zu < %zu", workspace_bytes, pb);
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
