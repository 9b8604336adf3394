// ttx_tt_bags_bf16.hip -- the POOLED bf16 inference forward of a three-core TT table in one launch: bag-major, no plan, no sort, no
// workspace, no rows.  Pooling is linear and the MFMA accumulates, so a wave that walks a bag's lookups runs product 2 of every
// lookup into the SAME fp32 accumulators; per_sample_weights are a multiply and padding_idx a skip inside that walk.  Packed cores:
// the MFMA-tail layout of ttx_tt_bf16m.hip, unchanged.  include/ttx.h "bf16 inference forward, pooled in one launch"; DESIGN.md 4.25.
//
// One work-group of 256 threads per bag (grid = nb); the table of bag b is b / (nb / num_tables).  Wave w takes the bag's slots
// w, w + 4, .. in slot order; everything a wave touches in LDS during the walk is its own region, so the walk has no work-group
// barrier.  A slot whose index equals padding_idx is skipped whole (nothing decoded, nothing loaded, not counted for the mean).
// Per live lookup, per wave:
//   product 1   x_0^T: M = the core-1 columns (b, k2) in tiles of 16, N = a (q0 padded to 16), K = k1.  A = the lookup's packed
//               core-1 slice, streamed from L2 one M tile ahead of the MFMAs; B = its core-0 slice (lanes with a >= q0 supply zero
//               and load nothing).  A lane's four accumulators are k2 = 16 t + 4 (l >> 4) .. + 3 of row (a, b), a = l & 15:
//               multiplied by the lookup's weight in fp32, rounded ONCE to bf16 (nearest even) and written as one 8-byte LDS store
//               into the wave's x_0 tile X[(a, b)][K2p].
//   product 2   M = the rows (a, b) (<= 4 tiles of 16), N = c (Q2P = 16 or 32), K = k2.  A = X (one ds_read_b128 per K block),
//               B = the lookup's transposed core-2 slice.  The accumulators are NOT cleared between lookups: after the walk they
//               hold the wave's share of the bag sum.
// The next slot's core-0 / core-2 fragments and first core-1 tile are requested before the current lookup's MFMAs, and the index
// and weight of the slot after that: the dependent chain index -> slices -> MFMA -> LDS -> MFMA of one lookup runs beside the
// loads of the next.
// X (bf16): row rho = a q1 + b at rho S bytes, S = 2 (K2p + 8): S / 16 = K2p / 8 + 1 is odd, so the 16 rows of a product-2 read
// (16 lanes of one l >> 4, S apart) fall on the 16 different 16-byte bank groups of the 64 x 4-byte banks: conflict-free for every
// tile (DESIGN.md 4.25 for the stores).  Columns [16 ceil(r2 / 16), K2p) are written by nobody else: zeroed once per wave.
// Combine: each wave writes its accumulators into its own region as [D] floats, ONE barrier, then element e is summed in wave
// order 0, 1, 2, 3 by its fixed owner (thread e / 4 mod 256 for 16-byte stores, e mod 256 otherwise), divided by max(1, live) for
// the mean, and written once.  No atomics, one writer per element: bit-identical from run to run, capturable.
#include "ttx_internal.h"

namespace ttx {
namespace {

constexpr int kBgThreads = 256;
constexpr int kBgWaves = kBgThreads / kWave;
constexpr int kBgMaxRank = 64;   // r1, r2: KB, K2B <= 2
constexpr int kBgMaxRows = 64;   // q0 q1: <= 4 M tiles of product 2, the bag accumulators in registers
constexpr int kBgMaxQ2 = 32;
constexpr int kBgMT2 = kBgMaxRows / 16;

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// everything the kernel needs of a geometry (host-derived; travels by value)
struct BgShape {
  int q0, q1, q2, r2;
  int MT, nm;     // M tiles of a q1 block in product 1: ceil(r2 / 16); of a lookup: q1 MT
  int R, NT2;     // rows (a, b) of a lookup, M tiles of product 2
  int S;          // bytes between rows of X
  int D;
  int p0, p1, p2;
  int pe0, pe1, pe2;  // packed bf16 elements of a slice of core t
  int region;     // bytes of a wave's LDS region: max(X, its [D] floats of the combine)
  int vec;        // 16-byte output stores
};

// host-only, stateless.  false: not a shape of this kernel.
bool bg_shape(const ttx_geom* g, BgShape* o) {
  if (!g || g->T != 3 || !ttx_tt_rows_bf16m_supported(g)) return false;
  if (g->p_tables && g->num_tables > 1) return false;  // (no plan: the kernel decodes indices itself, by ONE p)
  const int r1 = g->r[1], r2 = g->r[2];
  if (r1 > kBgMaxRank || r2 > kBgMaxRank || g->q[0] > 16 || g->q[0] * g->q[1] > kBgMaxRows || g->q[2] > kBgMaxQ2) return false;
  BgShape s;
  memset(&s, 0, sizeof(s));
  s.q0 = g->q[0]; s.q1 = g->q[1]; s.q2 = g->q[2]; s.r2 = r2;
  const int K1p = (r1 + 31) / 32 * 32, K2p = (r2 + 31) / 32 * 32;
  s.MT = (r2 + 15) / 16;
  s.nm = s.q1 * s.MT;
  s.R = s.q0 * s.q1;
  s.NT2 = (s.R + 15) / 16;
  s.S = 2 * (K2p + 8);
  s.D = s.R * s.q2;
  s.p0 = g->p[0]; s.p1 = g->p[1]; s.p2 = g->p[2];
  s.pe0 = s.q0 * K1p;
  s.pe1 = (s.q1 * r2 + 15) / 16 * 16 * K1p;
  s.pe2 = (s.q2 + 15) / 16 * 16 * K2p;
  const int x = s.R * s.S, c = 4 * s.D;
  s.region = ((x > c ? x : c) + 15) / 16 * 16;
  if (o) *o = s;
  return true;
}

// two fp32 -> two bf16 in one dword, round to nearest even (gfx950: one v_cvt_pk_bf16_f32)
__device__ __forceinline__ unsigned pk_bf16(float lo, float hi) {
  const f32x2 v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// the A fragments of product 1's M tile mt = b MT + t: column k2 = 16 t + (l & 15) of q1 block b, k = 8 (l >> 4) .. + 7 of every
// 32; zero where the tile or the column does not exist (nothing is read there)
template <int KB>
__device__ __forceinline__ void load_a1(uint4 (&af)[KB], const unsigned short* __restrict__ base1, int mt, const BgShape& sh, int li,
                                        int lg) {
  const int b = mt / sh.MT;
  const int k2 = 16 * (mt - b * sh.MT) + li;
  const bool ok = mt < sh.nm && k2 < sh.r2;
  const unsigned short* ap = base1 + (size_t)(ok ? b * sh.r2 + k2 : 0) * (KB * 32) + 8 * lg;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) af[kb] = ok ? *(const uint4*)(ap + kb * 32) : make_uint4(0, 0, 0, 0);
}

// what a wave holds of one lookup before its MFMAs
template <int KB, int K2B, int MQ>
struct BgFrag {
  uint4 b0[KB];       // core 0: row a = l & 15, k1 = 8 (l >> 4) .. + 7 of every 32
  uint4 a1[KB];       // core 1: M tile 0
  uint4 c2[MQ][K2B];  // core 2: row c = 16 nq + (l & 15), k2 = 8 (l >> 4) .. + 7 of every 32
  const unsigned short* base1;
};

// decode with the clamps of TTInferenceBag._rows_torch (negative -> 0, i0 <= p0 - 1) and request the lookup's fragments
template <int KB, int K2B, int MQ>
__device__ __forceinline__ void fetch(BgFrag<KB, K2B, MQ>& f, long long idx, int tab, const BgShape& sh,
                                      const unsigned short* __restrict__ c0, const unsigned short* __restrict__ c1,
                                      const unsigned short* __restrict__ c2, int li, int lg) {
  const unsigned long long u = idx < 0 ? 0ull : (unsigned long long)idx;
  unsigned long long rest;
  int i2;
  if ((u >> 32) == 0) {  // (wave-uniform: the 32-bit divisions of nearly every table)
    const unsigned v = (unsigned)u, d = v / (unsigned)sh.p2;
    i2 = (int)(v - d * (unsigned)sh.p2);
    rest = d;
  } else {
    rest = u / (unsigned long long)sh.p2;
    i2 = (int)(u - rest * (unsigned long long)sh.p2);
  }
  const unsigned long long hi = rest / (unsigned long long)sh.p1;
  const int i1 = (int)(rest - hi * (unsigned long long)sh.p1);
  const int i0 = hi < (unsigned long long)sh.p0 ? (int)hi : sh.p0 - 1;
  const size_t s0 = (size_t)tab * sh.p0 + i0, s1 = (size_t)tab * sh.p1 + i1, s2 = (size_t)tab * sh.p2 + i2;
  const unsigned short* bp = c0 + s0 * sh.pe0 + (li < sh.q0 ? li : 0) * (KB * 32) + 8 * lg;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) f.b0[kb] = li < sh.q0 ? *(const uint4*)(bp + kb * 32) : make_uint4(0, 0, 0, 0);
  f.base1 = c1 + s1 * sh.pe1;
  load_a1<KB>(f.a1, f.base1, 0, sh, li, lg);
  const unsigned short* cp = c2 + s2 * sh.pe2 + li * (K2B * 32) + 8 * lg;  // (16 nq + li < Q2P: inside the packed slice)
#pragma unroll
  for (int nq = 0; nq < MQ; ++nq)
#pragma unroll
    for (int kb = 0; kb < K2B; ++kb) f.c2[nq][kb] = *(const uint4*)(cp + nq * 16 * (K2B * 32) + kb * 32);
}

template <int KB, int K2B, int MQ>
__device__ __forceinline__ void no_frag(BgFrag<KB, K2B, MQ>& f, const unsigned short* c1) {
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) f.b0[kb] = f.a1[kb] = make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int nq = 0; nq < MQ; ++nq)
#pragma unroll
    for (int kb = 0; kb < K2B; ++kb) f.c2[nq][kb] = make_uint4(0, 0, 0, 0);
  f.base1 = c1;
}

template <int KB, int K2B, int MQ>  // KB = K1p / 32, K2B = K2p / 32, MQ = Q2P / 16
__global__ __launch_bounds__(kBgThreads) void tt_bags_bf16_kernel(const long long* __restrict__ indices,
                                                                  const long long* __restrict__ offsets,
                                                                  const float* __restrict__ weights, long long padding_idx, int mean,
                                                                  long long nnz, long long bags_per_table, BgShape sh,
                                                                  const unsigned short* __restrict__ c0,
                                                                  const unsigned short* __restrict__ c1,
                                                                  const unsigned short* __restrict__ c2, float* __restrict__ output) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int li = lane & 15, lg = lane >> 4;
  unsigned char* X = smem + (size_t)wave * sh.region;       // this wave's x_0 tile; after the walk its [D] partial sums
  int* lives = (int*)(smem + (size_t)kBgWaves * sh.region);  // [4] live lookups of each wave
  const long long bag = blockIdx.x;
  const int tab = (int)(bag / bags_per_table);
  // (the offsets are not trusted for memory safety: the bag is cut to [0, nnz))
  long long beg = offsets[bag], end = offsets[bag + 1];
  beg = beg < 0 ? 0 : (beg > nnz ? nnz : beg);
  end = end < beg ? beg : (end > nnz ? nnz : end);
  const bool pad_on = padding_idx >= 0;
  // the columns product 1 never writes: 16 bf16 at [16 MT, K2p) of every row (a stale NaN there times core 2's zero padding is a
  // NaN); this wave's own rows, read by this wave only
  if (16 * sh.MT < K2B * 32)
    for (int e = lane; e < 2 * sh.R; e += kWave) *(uint4*)(X + (size_t)(e >> 1) * sh.S + 32 * sh.MT + 16 * (e & 1)) = make_uint4(0, 0, 0, 0);

  f32x4 acc[kBgMT2][MQ];
#pragma unroll
  for (int mt = 0; mt < kBgMT2; ++mt)
#pragma unroll
    for (int nq = 0; nq < MQ; ++nq) acc[mt][nq] = f32x4{0.f, 0.f, 0.f, 0.f};
  int live = 0;

  long long s = beg + wave;
  BgFrag<KB, K2B, MQ> cur;
  bool live_c = false;
  float w_c = 1.f;
  if (s < end) {
    const long long idx = indices[s];
    live_c = !(pad_on && idx == padding_idx);
    if (weights) w_c = weights[s];
    if (live_c) fetch<KB, K2B, MQ>(cur, idx, tab, sh, c0, c1, c2, li, lg);
  }
  if (!live_c) no_frag<KB, K2B, MQ>(cur, c1);
  bool has_n = s + kBgWaves < end;
  long long idx_n = has_n ? indices[s + kBgWaves] : 0;
  float w_n = (has_n && weights) ? weights[s + kBgWaves] : 1.f;

  for (; s < end; s += kBgWaves) {  // (wave-uniform throughout)
    // the index and weight two slots ahead, the fragments one slot ahead: all requested before this lookup's MFMAs
    const bool has_nn = s + 2 * kBgWaves < end;
    const long long idx_nn = has_nn ? indices[s + 2 * kBgWaves] : 0;
    const float w_nn = (has_nn && weights) ? weights[s + 2 * kBgWaves] : 1.f;
    const bool live_n = has_n && !(pad_on && idx_n == padding_idx);
    BgFrag<KB, K2B, MQ> nxt;
    if (live_n)
      fetch<KB, K2B, MQ>(nxt, idx_n, tab, sh, c0, c1, c2, li, lg);
    else
      no_frag<KB, K2B, MQ>(nxt, c1);
    if (live_c) {
      ++live;
      // ---- product 1: the M tiles (b, t) of the lookup, the next tile's fragments in flight beside this tile's MFMAs
      uint4 af[KB];
#pragma unroll
      for (int kb = 0; kb < KB; ++kb) af[kb] = cur.a1[kb];
      for (int mt = 0; mt < sh.nm; ++mt) {
        uint4 an[KB];
        load_a1<KB>(an, cur.base1, mt + 1, sh, li, lg);
        f32x4 x = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KB; ++kb)
          x = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[kb]), __builtin_bit_cast(bf16x8, cur.b0[kb]), x, 0,
                                                      0, 0);
        const int b = mt / sh.MT;
        if (li < sh.q0)  // (row li q1 + b < R, column 16 t + 4 lg + 3 < 16 MT <= K2p: inside the wave's X)
          *(uint2*)(X + (size_t)(li * sh.q1 + b) * sh.S + 2 * (16 * (mt - b * sh.MT) + 4 * lg)) =
              make_uint2(pk_bf16(x[0] * w_c, x[1] * w_c), pk_bf16(x[2] * w_c, x[3] * w_c));
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) af[kb] = an[kb];
      }
      // (one wave writes and reads X: the LDS serves a wave's accesses in order; the fences keep the compiler from moving them)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      // ---- product 2: into the bag's accumulators
#pragma unroll
      for (int mt = 0; mt < kBgMT2; ++mt) {
        if (mt < sh.NT2) {
          const int rr = min(16 * mt + li, sh.R - 1);  // (a row past the lookup's last reads the last: no read leaves X)
          const unsigned char* xr = X + (size_t)rr * sh.S + 16 * lg;
#pragma unroll
          for (int kb = 0; kb < K2B; ++kb) {
            const uint4 xv = *(const uint4*)(xr + 64 * kb);
#pragma unroll
            for (int nq = 0; nq < MQ; ++nq)
              acc[mt][nq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, xv),
                                                                    __builtin_bit_cast(bf16x8, cur.c2[nq][kb]), acc[mt][nq], 0, 0, 0);
          }
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();  // (the next lookup's stores into X stay behind these reads)
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    cur = nxt;
    live_c = live_n;
    w_c = w_n;
    idx_n = idx_nn;
    w_n = w_nn;
    has_n = has_nn;
  }

  // ---- combine: the wave's share as [D] floats in its own region (a lane holds rows 16 mt + 4 lg + i of column c = 16 nq + li)
  float* part = (float*)X;
#pragma unroll
  for (int mt = 0; mt < kBgMT2; ++mt)
#pragma unroll
    for (int nq = 0; nq < MQ; ++nq)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int rho = 16 * mt + 4 * lg + i, c = 16 * nq + li;
        if (rho < sh.R && c < sh.q2) part[rho * sh.q2 + c] = acc[mt][nq][i];  // (rho q2 + c < D <= region / 4)
      }
  if (lane == 0) lives[wave] = live;
  __syncthreads();
  const int n_live = lives[0] + lives[1] + lives[2] + lives[3];
  const float div = (float)(n_live > 1 ? n_live : 1);
  const float* p0 = (const float*)smem;
  const int rs = sh.region / 4;
  float* out = output + (size_t)bag * sh.D;
  if (sh.vec) {  // (q2 % 4 == 0 and output 16-byte aligned: D % 4 == 0, every piece aligned)
    for (int e = 4 * tid; e < sh.D; e += 4 * kBgThreads) {
      float4 v = *(const float4*)(p0 + e);
#pragma unroll
      for (int w = 1; w < kBgWaves; ++w) {
        const float4 u = *(const float4*)(p0 + w * rs + e);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      if (mean) { v.x /= div; v.y /= div; v.z /= div; v.w /= div; }
      *(float4*)(out + e) = v;
    }
  } else {
    for (int e = tid; e < sh.D; e += kBgThreads) {
      float v = p0[e];
#pragma unroll
      for (int w = 1; w < kBgWaves; ++w) v += p0[w * rs + e];
      out[e] = mean ? v / div : v;
    }
  }
}

template <int KB, int K2B, int MQ>
int launch_bags(const BgShape& sh, long long nb, long long nnz, const int64_t* indices, const int64_t* offsets, const float* weights,
                long long padding_idx, int mean, long long bags_per_table, const unsigned short* const* pc, float* output,
                hipStream_t st) {
  const int lds = kBgWaves * sh.region + 16;  // (<= 4 x 9216 + 16: below the 48 KiB every kernel may ask for)
  hipLaunchKernelGGL((tt_bags_bf16_kernel<KB, K2B, MQ>), dim3((unsigned)nb), dim3(kBgThreads), lds, st, (const long long*)indices,
                     (const long long*)offsets, weights, padding_idx, mean, nnz, bags_per_table, sh, pc[0], pc[1], pc[2], output);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

template <int KB, int K2B, typename... A>
int launch_bags_mq(const BgShape& sh, A... a) {
  return sh.q2 <= 16 ? launch_bags<KB, K2B, 1>(sh, a...) : launch_bags<KB, K2B, 2>(sh, a...);
}

}  // namespace
}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_tt_bags_bf16_supported(const ttx_geom* g) { return bg_shape(g, nullptr) ? 1 : 0; }

int ttx_tt_bags_bf16(const ttx_geom* g, int32_t D, int64_t nb, int64_t nnz, const int64_t* indices, const int64_t* offsets,
                     const float* per_sample_weights, int64_t padding_idx, int32_t mean, const void* const* packed_cores,
                     float* output, ttx_stream_t stream) {
  if (!g) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: geometry is NULL");
  BgShape sh;
  if (!bg_shape(g, &sh))
    TTX_FAIL(TTX_EUNSUPPORTED,
             "tt_bags_bf16: not a shape of the pooled bf16 kernel (T = 3, a shape of tt_rows_bf16m, ranks <= %d, q0 <= 16, q0 q1 <= %d, "
             "q2 <= %d, one p for every table: no p_tables)",
             kBgMaxRank, kBgMaxRows, kBgMaxQ2);
  Dims d;
  const int rc = make_dims(g, &d);
  if (rc) return rc;
  if (D != d.D) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: D=%d does not match prod(q)=%d", D, d.D);
  if (nb < 0 || nb >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: nb=%lld out of range", (long long)nb);
  if (nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: nnz=%lld out of range", (long long)nnz);
  if (nb % g->num_tables != 0)
    TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: nb=%lld bags is not a multiple of num_tables=%d", (long long)nb, g->num_tables);
  if (per_sample_weights && mean) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: per_sample_weights go with the sum, not with the mean");
  if (padding_idx < -1) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: padding_idx=%lld (-1: none)", (long long)padding_idx);
  if (nb == 0) return TTX_OK;
  if (!offsets || !output || (nnz > 0 && !indices)) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: NULL indices / offsets / output");
  if (!packed_cores || !packed_cores[0] || !packed_cores[1] || !packed_cores[2]) TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: NULL packed cores");
  if ((((uintptr_t)packed_cores[0]) | ((uintptr_t)packed_cores[1]) | ((uintptr_t)packed_cores[2])) & 15)
    TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: packed cores must be 16-byte aligned");
  if (((((uintptr_t)indices) | ((uintptr_t)offsets)) & 7) || ((((uintptr_t)per_sample_weights) | ((uintptr_t)output)) & 3))
    TTX_FAIL(TTX_EINVAL, "tt_bags_bf16: indices / offsets must be 8-byte, per_sample_weights / output 4-byte aligned");
  sh.vec = (sh.q2 % 4 == 0 && (((uintptr_t)output) & 15) == 0) ? 1 : 0;
  const unsigned short* pc[3] = {(const unsigned short*)packed_cores[0], (const unsigned short*)packed_cores[1],
                                 (const unsigned short*)packed_cores[2]};
  const long long bpt = nb / g->num_tables;
  hipStream_t st = (hipStream_t)stream;
  const int KB = (g->r[1] + 31) / 32, K2B = (g->r[2] + 31) / 32;
  if (KB == 1)
    return K2B == 1 ? launch_bags_mq<1, 1>(sh, (long long)nb, (long long)nnz, indices, offsets, per_sample_weights, (long long)padding_idx,
                                           (int)mean, bpt, pc, output, st)
                    : launch_bags_mq<1, 2>(sh, (long long)nb, (long long)nnz, indices, offsets, per_sample_weights, (long long)padding_idx,
                                           (int)mean, bpt, pc, output, st);
  return K2B == 1 ? launch_bags_mq<2, 1>(sh, (long long)nb, (long long)nnz, indices, offsets, per_sample_weights, (long long)padding_idx,
                                         (int)mean, bpt, pc, output, st)
                  : launch_bags_mq<2, 2>(sh, (long long)nb, (long long)nnz, indices, offsets, per_sample_weights, (long long)padding_idx,
                                         (int)mean, bpt, pc, output, st);
}

}  // extern "C"
