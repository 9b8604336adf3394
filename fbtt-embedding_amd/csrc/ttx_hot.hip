// ttx_hot.hip -- the serving-side hot row table of TTInferenceBag (include/ttx.h "hot rows of the inference forward"; DESIGN.md
// 4.23; not in the reference).  gfx950, wave64.
//
// A frozen module keeps its K most visited rows expanded, as bf16, beside the packed cores: hot_keys [K] int64 ascending (key =
// table * key_stride + index) and hot_rows [K, D] bf16.  A served batch is split on the device: ttx_hot_probe_pool looks every slot
// up in the table, pools the rows of the hits per bag and masks them out of the index array; ttx_bags_compact drops the masked
// slots; the misses are planned and contracted as ever; ttx_bag_sum_pool_add sums a bag's miss rows on top of its hit sum.
//
// Probe + pool: one wave per bag.  The wave first probes up to 64 slots of the bag at once, one slot per lane: a branch-free
// lower-bound search whose step count depends on K alone, so every step is ONE round of 64 loads from an array that stays in L2,
// and every address lies inside the array whatever the key.  The slot numbers (-1: miss) then travel by wave shuffle to the lane
// layout of dense_fwd_kernel (ttx_dense.hip): LPR lanes per row, 64 / LPR row groups, four rows of a group in flight; a row is
// read as 16-byte loads of 8 bf16, widened by a shift and accumulated in fp32 in slot order; the groups are combined by xor
// shuffles.  Plain loads and stores, one writer per element, nothing read back: bit-identical from run to run, capturable.
#include "ttx_internal.h"

namespace ttx {

constexpr int kHotThreads = 256;
constexpr int kHotWaves = kHotThreads / kWave;  // bags in flight per work-group
constexpr int kHotFlight = 4;                   // rows of a lane group in flight

__device__ __forceinline__ long long hot_clamp(long long v, long long nnz) { return v < 0 ? 0 : (v > nnz ? nnz : v); }

// v[0 .. W) = the W bf16 at p, widened exactly (a bf16 is the upper half of its fp32)
template <int W>
__device__ __forceinline__ void hot_ld(const unsigned short* p, float (&v)[W]) {
  if constexpr (W == 8) {
    const uint4 t = *(const uint4*)p;
    const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      v[2 * k] = __uint_as_float(w[k] << 16);
      v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u);
    }
  } else {
    v[0] = __uint_as_float((unsigned)*p << 16);
  }
}

template <int W>
__device__ __forceinline__ void hot_st(float* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
    *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
  } else {
    p[0] = v[0];
  }
}

// The table slot of `key`, or -1: lower bound over keys[0 .. K), K >= 1, strictly ascending.  The search range [base, base + len)
// halves whatever the comparison says, so the loop runs floor(log2 K) + 1 times for every lane alike and reads keys[base + half - 1]
// with base + half <= K throughout.
__device__ __forceinline__ int hot_find(const int64_t* __restrict__ keys, int K, long long key) {
  int base = 0;
  for (int len = K; len > 1;) {
    const int half = len >> 1;
    base = keys[base + half - 1] < key ? base + half : base;
    len -= half;
  }
  return keys[base] == key ? base : -1;
}

// W bf16 per lane (8: 16-byte loads, D % 8 == 0; 1: the scalar path), DV = D / W column vectors; rows wider than a wave's LPR
// vectors are walked per column block, the probe with them (masked is written by the first block only).  A wave takes the bags
// bag, bag + waves of the grid, ...; the waves of bag 0 and of bag nb - 1 also mask the slots that no bag covers.
template <int W>
__global__ __launch_bounds__(kHotThreads) void hot_probe_pool_kernel(long long nb, long long B, int DV, int lpr_log2, long long nnz,
                                                                    const int64_t* __restrict__ indices,
                                                                    const int64_t* __restrict__ offsets, long long key_stride, int K,
                                                                    const int64_t* __restrict__ keys,
                                                                    const unsigned short* __restrict__ hot_rows,
                                                                    int64_t* __restrict__ masked, float* __restrict__ hit_sum) {
  const int lane = lane_id();
  const int LPR = 1 << lpr_log2, G = kWave >> lpr_log2;
  const int grp = lane >> lpr_log2, cl = lane & (LPR - 1);
  const size_t ld = (size_t)DV * W;
  for (long long bag = (long long)blockIdx.x * kHotWaves + threadIdx.x / kWave; bag < nb; bag += (long long)gridDim.x * kHotWaves) {
    const long long first = (bag / B) * key_stride;  // key of the table's index 0
    const long long s = hot_clamp(offsets[bag], nnz);
    long long e = hot_clamp(offsets[bag + 1], nnz);
    e = e < s ? s : e;
    if (bag == 0)
      for (long long j = lane; j < s; j += kWave) masked[j] = -1;
    if (bag == nb - 1)
      for (long long j = e + lane; j < nnz; j += kWave) masked[j] = -1;
    for (int c0 = 0; c0 < DV; c0 += LPR) {
      const int c = c0 + cl;
      const bool colok = c < DV;
      const unsigned short* rcol = hot_rows + (size_t)(colok ? c : 0) * W;
      float m[W];
#pragma unroll
      for (int k = 0; k < W; ++k) m[k] = 0.f;
      for (long long r0 = s; r0 < e; r0 += kWave) {  // a round: 64 slots probed at once
        const long long j = r0 + lane;
        const bool valid = j < e;
        long long idx = 0;
        if (valid) idx = indices[j];
        int slot = -1;
        if (K > 0) {  // (wave-uniform)
          const bool inside = valid && idx >= 0 && idx < key_stride;
          const int f = hot_find(keys, K, inside ? first + idx : 0);
          slot = inside ? f : -1;
        }
        if (valid && c0 == 0) masked[j] = slot >= 0 ? -1 : (idx < 0 ? 0 : idx);
        const int cnt = (int)(e - r0 < kWave ? e - r0 : kWave);
        for (int u0 = 0; u0 < cnt; u0 += kHotFlight * G) {  // (wave-uniform: every lane takes part in the shuffles)
          float a[kHotFlight][W];
#pragma unroll
          for (int u = 0; u < kHotFlight; ++u) {
            const int src = u0 + u * G + grp;
            const int sl = __shfl(slot, src & (kWave - 1), kWave);
#pragma unroll
            for (int k = 0; k < W; ++k) a[u][k] = 0.f;
            if (src < cnt && sl >= 0 && colok) hot_ld<W>(rcol + (size_t)sl * ld, a[u]);
          }
#pragma unroll
          for (int u = 0; u < kHotFlight; ++u)
#pragma unroll
            for (int k = 0; k < W; ++k) m[k] += a[u][k];
        }
      }
      for (int o = LPR; o < kWave; o <<= 1) {  // combine the row groups
#pragma unroll
        for (int k = 0; k < W; ++k) m[k] += __shfl_xor(m[k], o, kWave);
      }
      if (grp == 0 && colok) hot_st<W>(hit_sum + (size_t)bag * ld + (size_t)c * W, m);
    }
  }
}

// output[b, :] = addend[b, :] + rows[offsets[b]] + rows[offsets[b] + 1] + ... in index order: bag_sum_pool_kernel (ttx_tt_bf16.hip)
// started from the addend.  One thread per (bag, piece of the row) reads its addend and writes its output: output may be addend.
__device__ __forceinline__ void hot_add(float4& a, const float4 v) { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
__device__ __forceinline__ void hot_add(float& a, const float v) { a += v; }

template <typename V>
__global__ __launch_bounds__(256) void bag_sum_pool_add_kernel(long long nb, int DP, const int64_t* __restrict__ offsets,
                                                               const V* __restrict__ rows, const V* addend, V* out) {
  const long long total = nb * DP;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += stride) {
    const long long bag = e / DP;
    const int c = (int)(e - bag * DP);
    long long a = offsets[bag], z = offsets[bag + 1];
    a = a < 0 ? 0 : a;
    V acc = addend[e];
    const V* p = rows + a * DP + c;
    long long j = a;
    for (; j + 3 < z; j += 4, p += 4 * (long long)DP) {  // four rows in flight, added in index order
      const V v0 = p[0], v1 = p[DP], v2 = p[2 * (long long)DP], v3 = p[3 * (long long)DP];
      hot_add(acc, v0); hot_add(acc, v1); hot_add(acc, v2); hot_add(acc, v3);
    }
    for (; j < z; ++j, p += DP) hot_add(acc, p[0]);
    out[e] = acc;
  }
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_hot_probe_pool(int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* offsets,
                       int64_t key_stride, int64_t K, const int64_t* hot_keys, const void* hot_rows_bf16, int64_t* masked_indices,
                       float* hit_sum, ttx_stream_t stream) {
  if (num_tables <= 0 || B < 0 || D <= 0 || nnz < 0 || K < 0 || key_stride <= 0)
    TTX_FAIL(TTX_EINVAL, "hot_probe_pool: bad num_tables / B / D / nnz / K / key_stride (%d, %lld, %d, %lld, %lld, %lld)", num_tables,
             (long long)B, D, (long long)nnz, (long long)K, (long long)key_stride);
  if (nnz >= (1ll << 31) || K >= (1ll << 31) || (long long)num_tables * B >= (1ll << 31))
    TTX_FAIL(TTX_EINVAL, "hot_probe_pool: nnz, K and num_tables * B must be below 2^31");
  if (key_stride > (1ll << 62) / num_tables) TTX_FAIL(TTX_EINVAL, "hot_probe_pool: num_tables * key_stride beyond 2^62");
  const long long nb = (long long)num_tables * B;
  if (nb == 0 || nnz == 0) return TTX_OK;
  if (!indices || !offsets || !masked_indices || !hit_sum) TTX_FAIL(TTX_EINVAL, "hot_probe_pool: NULL indices / offsets / output");
  if (K > 0 && (!hot_keys || !hot_rows_bf16)) TTX_FAIL(TTX_EINVAL, "hot_probe_pool: NULL hot_keys / hot_rows with K > 0");
  if ((((uintptr_t)indices) | ((uintptr_t)offsets) | ((uintptr_t)hot_keys) | ((uintptr_t)masked_indices)) & 7)
    TTX_FAIL(TTX_EINVAL, "hot_probe_pool: indices, offsets, hot_keys and masked_indices must be 8-byte aligned");
  if ((((uintptr_t)hit_sum) & 3) || (((uintptr_t)hot_rows_bf16) & 1))
    TTX_FAIL(TTX_EINVAL, "hot_probe_pool: hit_sum must be 4-byte, hot_rows 2-byte aligned");
  const long long blocks = (nb + kHotWaves - 1) / kHotWaves;
  const dim3 grid((unsigned)(blocks < (1ll << 16) ? blocks : (1ll << 16)));
  const unsigned short* hr = (const unsigned short*)hot_rows_bf16;
  const bool v8 = D % 8 == 0 && ((((uintptr_t)hot_rows_bf16) | ((uintptr_t)hit_sum)) & 15) == 0;
  const int DV = v8 ? D / 8 : D;
  int lg = 0;  // lanes per row: the column vectors rounded up to a power of two, at most a wave
  while ((1 << lg) < DV && (1 << lg) < kWave) ++lg;
  if (v8)
    hipLaunchKernelGGL(hot_probe_pool_kernel<8>, grid, dim3(kHotThreads), 0, (hipStream_t)stream, nb, (long long)B, DV, lg,
                       (long long)nnz, indices, offsets, (long long)key_stride, (int)K, hot_keys, hr, masked_indices, hit_sum);
  else
    hipLaunchKernelGGL(hot_probe_pool_kernel<1>, grid, dim3(kHotThreads), 0, (hipStream_t)stream, nb, (long long)B, DV, lg,
                       (long long)nnz, indices, offsets, (long long)key_stride, (int)K, hot_keys, hr, masked_indices, hit_sum);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_bag_sum_pool_add(int64_t nb, int32_t D, const int64_t* offsets, const float* rows, const float* addend, float* output,
                         ttx_stream_t stream) {
  if (nb < 0 || D <= 0 || nb >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bag_sum_pool_add: bad nb / D (nb=%lld, D=%d)", (long long)nb, D);
  if (nb == 0) return TTX_OK;
  if (!offsets || !rows || !addend || !output) TTX_FAIL(TTX_EINVAL, "bag_sum_pool_add: NULL input / output");
  if ((((uintptr_t)rows) | ((uintptr_t)addend) | ((uintptr_t)output)) & 3)
    TTX_FAIL(TTX_EINVAL, "bag_sum_pool_add: float pointers must be 4-byte aligned");
  if (((uintptr_t)offsets) & 7) TTX_FAIL(TTX_EINVAL, "bag_sum_pool_add: offsets must be 8-byte aligned");
  const bool v4 = D % 4 == 0 && ((((uintptr_t)rows) | ((uintptr_t)addend) | ((uintptr_t)output)) & 15) == 0;
  const int DP = v4 ? D / 4 : D;
  const long long blocks = (nb * DP + 255) / 256;
  const unsigned grid = (unsigned)(blocks < (1ll << 20) ? blocks : (1ll << 20));
  if (v4)
    hipLaunchKernelGGL(bag_sum_pool_add_kernel<float4>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)nb, DP, offsets,
                       (const float4*)rows, (const float4*)addend, (float4*)output);
  else
    hipLaunchKernelGGL(bag_sum_pool_add_kernel<float>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (long long)nb, DP, offsets, rows,
                       addend, output);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"
