// ttx_pool.hip -- nn.EmbeddingBag's "mean" and "max" pooling over per-lookup rows (not in the reference, which sums).
//
// The contraction kernels leave one row per lookup ([nnz, D], ttx_tt_rows_p); these kernels reduce them per bag and route
// the bag gradient back.  Plain loads and stores only: no atomics, every output element has one writer, so results are
// bit-identical from run to run and nothing is read back to the host (capturable).  Bags are described by `offsets`
// [nb + 1] int64 (closing entry included); bag b covers positions [offsets[b], offsets[b + 1]) of the batch.
#include "ttx_internal.h"

namespace ttx {

constexpr int kBagWaves = 4;  // bags (one wave each) per work-group
constexpr int kBagThreads = kBagWaves * kWave;

template <int W>
__device__ __forceinline__ void ld_vec(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    const float4 t = *(const float4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void st_vec(float* p, const float (&v)[W]) {
  if constexpr (W == 4) *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

template <int W>
__device__ __forceinline__ void ld_ivec(const int* p, int (&v)[W]) {
  if constexpr (W == 4) {
    const int4 t = *(const int4*)p;
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}

template <int W>
__device__ __forceinline__ void st_ivec(int* p, const int (&v)[W]) {
  if constexpr (W == 4) *(int4*)p = make_int4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// the extent of bag b, clamped to [0, nnz) (offsets past the batch read nothing)
__device__ __forceinline__ void bag_extent(const int64_t* __restrict__ offsets, long long b, long long nnz, long long* s,
                                           long long* e) {
  long long a = offsets[b], z = offsets[b + 1];
  a = a < 0 ? 0 : (a > nnz ? nnz : a);
  z = z < a ? a : (z > nnz ? nnz : z);
  *s = a;
  *e = z;
}

// Column-wise max of every bag and the position that holds it.  One wave per bag; W floats per lane (W = 4: float4 columns,
// W = 1: the scalar path for D % 4 != 0), DV = D / W column vectors.  Lane l works on column vector c0 + (l % LPR) of rows
// start + l / LPR, + G, + 2G, ... (LPR = 2^lpr_log2 lanes per row, G = 64 / LPR rows in flight); each lane keeps a running
// (max, position) per column with a STRICT > while it walks its rows in ascending order, so the first of equal values stays.
// The G row groups are then combined pairwise (xor shuffles), the lower position winning a tie: the result is the bag's
// lowest position among the maxima -- PyTorch's rule.  Rows wider than a wave's LPR vectors: the walk again per column block.
// Empty bag: output 0, argmax -1.
template <int W>
__global__ __launch_bounds__(kBagThreads) void bag_max_pool_kernel(long long nb, int DV, int lpr_log2, long long nnz,
                                                                   const int64_t* __restrict__ offsets,
                                                                   const float* __restrict__ rows, float* __restrict__ out,
                                                                   int* __restrict__ argmax) {
  const long long bag = (long long)blockIdx.x * kBagWaves + threadIdx.x / kWave;
  if (bag >= nb) return;  // (wave-uniform)
  const int lane = lane_id();
  const int LPR = 1 << lpr_log2, G = kWave >> lpr_log2;
  const int grp = lane >> lpr_log2, cl = lane & (LPR - 1);
  long long s, e;
  bag_extent(offsets, bag, nnz, &s, &e);
  const size_t ld = (size_t)DV * W;  // floats per row
  for (int c0 = 0; c0 < DV; c0 += LPR) {
    const int c = c0 + cl;
    const bool live = c < DV;
    float m[W];
    int p[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { m[k] = 0.f; p[k] = -1; }
    if (live) {
      const float* base = rows + (size_t)c * W;
      long long j = s + grp;
      for (; j + 3 * G < e; j += 4 * G) {  // four rows of the group in flight
        float a[4][W];
#pragma unroll
        for (int u = 0; u < 4; ++u) ld_vec<W>(base + (size_t)(j + u * G) * ld, a[u]);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int k = 0; k < W; ++k)
            if (p[k] < 0 || a[u][k] > m[k]) { m[k] = a[u][k]; p[k] = (int)(j + u * G); }
      }
      for (; j < e; j += G) {
        float a[W];
        ld_vec<W>(base + (size_t)j * ld, a);
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (p[k] < 0 || a[k] > m[k]) { m[k] = a[k]; p[k] = (int)j; }
      }
    }
    for (int o = LPR; o < kWave; o <<= 1) {  // combine the row groups (lanes that differ in the group bits)
#pragma unroll
      for (int k = 0; k < W; ++k) {
        const float om = __shfl_xor(m[k], o, kWave);
        const int op = __shfl_xor(p[k], o, kWave);
        if (op >= 0 && (p[k] < 0 || om > m[k] || (om == m[k] && op < p[k]))) { m[k] = om; p[k] = op; }
      }
    }
    if (grp == 0 && live) {
#pragma unroll
      for (int k = 0; k < W; ++k) m[k] = p[k] < 0 ? 0.f : m[k];
      st_vec<W>(out + (size_t)bag * ld + (size_t)c * W, m);
      st_ivec<W>(argmax + (size_t)bag * ld + (size_t)c * W, p);
    }
  }
}

// Gather form of the max backward: d_rows[n, e] = argmax[bag(n), e] == n ? d_output[bag(n), e] : 0 for every lookup n.  One wave
// per bag (the forward's lane layout): a lane loads its columns' winner and gradient once and writes them, or zeros, down the
// bag's rows.  Every element of d_rows is written exactly once with a plain store -- the lookups no bag covers (positions before
// offsets[0] or from offsets[nb] on) get zero rows from the first / last bag's wave.
template <int W>
__global__ __launch_bounds__(kBagThreads) void bag_max_pool_bwd_kernel(long long nb, int DV, int lpr_log2, long long nnz,
                                                                       const int64_t* __restrict__ offsets,
                                                                       const int* __restrict__ argmax,
                                                                       const float* __restrict__ d_output,
                                                                       float* __restrict__ d_rows) {
  const long long bag = (long long)blockIdx.x * kBagWaves + threadIdx.x / kWave;
  if (bag >= nb) return;
  const int lane = lane_id();
  const int LPR = 1 << lpr_log2, G = kWave >> lpr_log2;
  const int grp = lane >> lpr_log2, cl = lane & (LPR - 1);
  long long s, e;
  bag_extent(offsets, bag, nnz, &s, &e);
  long long head = 0, tail = nnz;  // uncovered positions: [0, head) by bag 0, [tail, nnz) by the last bag
  if (bag == 0) {
    long long s0, e0;
    bag_extent(offsets, 0, nnz, &s0, &e0);
    head = s0;
  }
  if (bag == nb - 1) tail = e;
  const size_t ld = (size_t)DV * W;
  for (int c0 = 0; c0 < DV; c0 += LPR) {
    const int c = c0 + cl;
    if (c >= DV) continue;
    int am[W];
    float gv[W], v[W], z[W];
    ld_ivec<W>(argmax + (size_t)bag * ld + (size_t)c * W, am);
    ld_vec<W>(d_output + (size_t)bag * ld + (size_t)c * W, gv);
#pragma unroll
    for (int k = 0; k < W; ++k) z[k] = 0.f;
    float* base = d_rows + (size_t)c * W;
    for (long long j = s + grp; j < e; j += G) {
#pragma unroll
      for (int k = 0; k < W; ++k) v[k] = am[k] == (int)j ? gv[k] : 0.f;
      st_vec<W>(base + (size_t)j * ld, v);
    }
    for (long long j = grp; j < head; j += G) st_vec<W>(base + (size_t)j * ld, z);
    for (long long j = tail + grp; j < nnz; j += G) st_vec<W>(base + (size_t)j * ld, z);
  }
}

// y[b, :] = x[b, :] / max(1, offsets[b + 1] - offsets[b]) -- the mean of a bag from its sum (forward) and the share of a bag's
// gradient that each of its lookups receives (backward).  y may be x.
template <int W>
__global__ __launch_bounds__(256) void bag_mean_scale_kernel(long long nb, int DV, const int64_t* __restrict__ offsets,
                                                            const float* x, float* y) {
  const long long total = nb * DV;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long b = i / DV;
    const long long cnt = offsets[b + 1] - offsets[b];
    const float d = (float)(cnt > 1 ? cnt : 1);
    float v[W];
    ld_vec<W>(x + (size_t)i * W, v);
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = v[k] / d;
    st_vec<W>(y + (size_t)i * W, v);
  }
}

__global__ __launch_bounds__(256) void iota64_kernel(long long n, int64_t* __restrict__ dst) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) dst[i] = i;
}

int fill_iota64(int64_t* dst, long long n, hipStream_t st) {
  if (n <= 0) return TTX_OK;
  const long long blocks = (n + 255) / 256;
  hipLaunchKernelGGL(iota64_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, n, dst);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

// W = 4 when D % 4 == 0 and every pointer is 16-byte aligned
static bool vec4_ok(int32_t D, std::initializer_list<const void*> ptrs) {
  if (D % 4 != 0) return false;
  for (const void* p : ptrs)
    if (((uintptr_t)p) & 15) return false;
  return true;
}

// log2 of the lanes per row: the column vectors rounded up to a power of two, at most a wave
static int lanes_log2(int DV) {
  int l = 0;
  while ((1 << l) < DV && (1 << l) < kWave) ++l;
  return l;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_bag_max_pool(int64_t nb, int32_t D, int64_t nnz, const int64_t* offsets, const float* rows, float* output,
                     int32_t* argmax, ttx_stream_t stream) {
  if (nb < 0 || D <= 0 || nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bag_max_pool: bad nb / D / nnz");
  if (nb == 0) return TTX_OK;
  if (!offsets || !output || !argmax || (nnz > 0 && !rows)) TTX_FAIL(TTX_EINVAL, "bag_max_pool: NULL input");
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((nb + kBagWaves - 1) / kBagWaves);
  if (vec4_ok(D, {rows, output, argmax})) {
    const int DV = D / 4;
    hipLaunchKernelGGL(bag_max_pool_kernel<4>, dim3(blocks), dim3(kBagThreads), 0, st, (long long)nb, DV, lanes_log2(DV),
                       (long long)nnz, offsets, rows, output, (int*)argmax);
  } else {
    hipLaunchKernelGGL(bag_max_pool_kernel<1>, dim3(blocks), dim3(kBagThreads), 0, st, (long long)nb, (int)D, lanes_log2(D),
                       (long long)nnz, offsets, rows, output, (int*)argmax);
  }
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_bag_max_pool_backward(int64_t nb, int32_t D, int64_t nnz, const int64_t* offsets, const int32_t* argmax,
                              const float* d_output, float* d_rows, ttx_stream_t stream) {
  if (nb < 0 || D <= 0 || nnz < 0 || nnz >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "bag_max_pool_backward: bad nb / D / nnz");
  if (nnz == 0) return TTX_OK;
  if (!d_rows) TTX_FAIL(TTX_EINVAL, "bag_max_pool_backward: NULL d_rows");
  hipStream_t st = (hipStream_t)stream;
  if (nb == 0) {  // (no bag: no lookup receives a gradient)
    TTX_HIP(hipMemsetAsync(d_rows, 0, (size_t)nnz * D * sizeof(float), st));
    return TTX_OK;
  }
  if (!offsets || !argmax || !d_output) TTX_FAIL(TTX_EINVAL, "bag_max_pool_backward: NULL input");
  const unsigned blocks = (unsigned)((nb + kBagWaves - 1) / kBagWaves);
  if (vec4_ok(D, {argmax, d_output, d_rows})) {
    const int DV = D / 4;
    hipLaunchKernelGGL(bag_max_pool_bwd_kernel<4>, dim3(blocks), dim3(kBagThreads), 0, st, (long long)nb, DV, lanes_log2(DV),
                       (long long)nnz, offsets, (const int*)argmax, d_output, d_rows);
  } else {
    hipLaunchKernelGGL(bag_max_pool_bwd_kernel<1>, dim3(blocks), dim3(kBagThreads), 0, st, (long long)nb, (int)D, lanes_log2(D),
                       (long long)nnz, offsets, (const int*)argmax, d_output, d_rows);
  }
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_bag_mean_scale(int64_t nb, int32_t D, const int64_t* offsets, const float* x, float* y, ttx_stream_t stream) {
  if (nb < 0 || D <= 0) TTX_FAIL(TTX_EINVAL, "bag_mean_scale: bad nb / D");
  if (nb == 0) return TTX_OK;
  if (!offsets || !x || !y) TTX_FAIL(TTX_EINVAL, "bag_mean_scale: NULL input");
  hipStream_t st = (hipStream_t)stream;
  const bool v4 = vec4_ok(D, {x, y});
  const long long total = nb * (v4 ? D / 4 : D);
  const long long blocks = (total + 255) / 256;
  const unsigned grid = (unsigned)(blocks < 8192 ? blocks : 8192);
  if (v4)
    hipLaunchKernelGGL(bag_mean_scale_kernel<4>, dim3(grid), dim3(256), 0, st, (long long)nb, D / 4, offsets, x, y);
  else
    hipLaunchKernelGGL(bag_mean_scale_kernel<1>, dim3(grid), dim3(256), 0, st, (long long)nb, (int)D, offsets, x, y);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"
