// ttx_rows_cache.hip -- rows of a cache-live unpooled lookup between partition order and positions (TTEmbedding(use_cache=True);
// not in the reference).
//
// The live preprocess (ttx_preprocess_indices_async) leaves the n live lookups of a batch of N positions in partition order:
// the misses in front, [0, n_tt), the hits behind them, [n_tt, n); pos[s] = part_rowidx[s] is the position of slot s,
// loc[s] = part_cache_locations[s] its cache row (-1 in front of n_tt).  The split point n_tt lives on the device (n_tt_dev)
// or comes from the host (n_tt_dev == NULL).  ttx_rows_place writes the output of the lookup -- out[pos[s], :] = the contracted
// row of a miss (rows_tt[s, :]) or the cache row of a hit (cache_weight[loc[s], :], gathered here: no rows buffer for the hits)
// -- and exact zeros at the padding positions (rank, as for ttx_rows_expand): pos being injective onto the live positions,
// every element of `out` has one writer and no memset runs in front.  ttx_rows_pick is the transpose for the misses only:
// d_rows[s, :] = d_out[pos[s], :], s < n_tt (the hits' gradient rows are read in place by the cache rows' update).
//
// Both move bytes and nothing else, tiled like ttx_rows.hip: a work-group takes a tile of R consecutive slots (place: slot s
// AND position s, n <= N) -- R chosen so that a tile holds about kPieces pieces, short rows grouped so that they still fill
// the waves -- and its threads walk the tile's pieces in order: a piece is 16 bytes (float4: D % 4 == 0 and every float pointer
// 16-byte aligned) or one float, consecutive lanes hold consecutive pieces of a row, kUnroll pieces per thread in flight.  The
// (slot, column) of a thread's next piece follows from the last one by an add and a compare.  Element offsets are 64-bit.  No
// atomics, no LDS, no workspace, nothing read back: bit-identical from run to run, capturable.
#include "ttx_internal.h"

namespace ttx {

constexpr int kRcThreads = 256;
constexpr int kRcUnroll = 4;
constexpr int kRcPieces = kRcThreads * kRcUnroll;  // pieces of a tile of short rows
constexpr long long kRcMaxBlocks = 1ll << 20;      // grid.x (tiles beyond it: the work-groups stride over them)

// the split point: *n_tt_dev (or the host's value) clamped to the n slots there are
__device__ __forceinline__ long long rc_split(const int32_t* __restrict__ n_tt_dev, int n_tt, long long n) {
  const long long v = n_tt_dev ? (long long)*n_tt_dev : (long long)n_tt;
  return v < 0 ? 0 : (v > n ? n : v);
}

template <typename V>
__device__ __forceinline__ void rc_place(long long N, long long n, int n_tt_host, const int32_t* __restrict__ n_tt_dev, int DP, int R,
                                         int step_r, int step_c, const int64_t* __restrict__ pos, const int32_t* __restrict__ loc,
                                         const V* __restrict__ rows_tt, const V* __restrict__ cache, long long cache_size,
                                         const int64_t* __restrict__ rank, V* __restrict__ out) {
  const long long n_tt = rc_split(n_tt_dev, n_tt_host, n);
  const long long tiles = (N + R - 1) / R;
  const unsigned tid = threadIdx.x;
  const int r_first = (int)(tid / (unsigned)DP), c_first = (int)(tid - (unsigned)r_first * (unsigned)DP);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i0 = tile * R;
    const int rows_here = (int)(N - i0 < R ? N - i0 : R);
    int r = r_first, c = c_first;
    while (r < rows_here) {
      V v[kRcUnroll];
      long long at[kRcUnroll];   // piece offset of slot s's row in `out`, -1: none
      long long zat[kRcUnroll];  // piece offset of the zero of padding position s, -1: none
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        at[u] = -1;
        zat[u] = -1;
        v[u] = V{};  // (every element assigned on every path: the arrays stay in registers)
        if (r < rows_here) {
          const long long s = i0 + r;
          if (s < n) {
            const long long p = pos[s];
            at[u] = (p < 0 ? 0 : (p > N - 1 ? N - 1 : p)) * DP + c;
            if (s < n_tt) {
              v[u] = rows_tt[s * DP + c];
            } else if (cache_size > 0) {
              const long long l = loc[s];
              v[u] = cache[(l < 0 ? 0 : (l > cache_size - 1 ? cache_size - 1 : l)) * DP + c];
            }
          }
          if (rank != nullptr) {
            if (!(rank[s + 1] > rank[s])) zat[u] = s * DP + c;
          }
        }
        r += step_r;
        c += step_c;
        if (c >= DP) { c -= DP; ++r; }
      }
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        if (at[u] >= 0) out[at[u]] = v[u];
        if (zat[u] >= 0) out[zat[u]] = V{};
      }
    }
  }
}

template <typename V>
__device__ __forceinline__ void rc_pick(long long N, long long n, int n_tt_host, const int32_t* __restrict__ n_tt_dev, int DP, int R,
                                        int step_r, int step_c, const int64_t* __restrict__ pos, const V* __restrict__ d_out,
                                        V* __restrict__ d_rows) {
  const long long n_tt = rc_split(n_tt_dev, n_tt_host, n);
  const long long tiles = (n_tt + R - 1) / R;
  const unsigned tid = threadIdx.x;
  const int r_first = (int)(tid / (unsigned)DP), c_first = (int)(tid - (unsigned)r_first * (unsigned)DP);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i0 = tile * R;
    const int rows_here = (int)(n_tt - i0 < R ? n_tt - i0 : R);
    int r = r_first, c = c_first;
    while (r < rows_here) {
      V v[kRcUnroll];
      long long at[kRcUnroll];  // piece offset of the store, -1: none
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u) {
        at[u] = -1;
        v[u] = V{};
        if (r < rows_here) {
          const long long s = i0 + r;
          const long long p = pos[s];
          at[u] = s * DP + c;
          v[u] = d_out[(p < 0 ? 0 : (p > N - 1 ? N - 1 : p)) * DP + c];
        }
        r += step_r;
        c += step_c;
        if (c >= DP) { c -= DP; ++r; }
      }
#pragma unroll
      for (int u = 0; u < kRcUnroll; ++u)
        if (at[u] >= 0) d_rows[at[u]] = v[u];
    }
  }
}

__global__ __launch_bounds__(kRcThreads) void rc_place4_kernel(long long N, long long n, int n_tt, const int32_t* __restrict__ n_tt_dev,
                                                               int DP, int R, int step_r, int step_c, const int64_t* __restrict__ pos,
                                                               const int32_t* __restrict__ loc, const float4* __restrict__ rows_tt,
                                                               const float4* __restrict__ cache, long long cache_size,
                                                               const int64_t* __restrict__ rank, float4* __restrict__ out) {
  rc_place<float4>(N, n, n_tt, n_tt_dev, DP, R, step_r, step_c, pos, loc, rows_tt, cache, cache_size, rank, out);
}

__global__ __launch_bounds__(kRcThreads) void rc_place1_kernel(long long N, long long n, int n_tt, const int32_t* __restrict__ n_tt_dev,
                                                               int DP, int R, int step_r, int step_c, const int64_t* __restrict__ pos,
                                                               const int32_t* __restrict__ loc, const float* __restrict__ rows_tt,
                                                               const float* __restrict__ cache, long long cache_size,
                                                               const int64_t* __restrict__ rank, float* __restrict__ out) {
  rc_place<float>(N, n, n_tt, n_tt_dev, DP, R, step_r, step_c, pos, loc, rows_tt, cache, cache_size, rank, out);
}

__global__ __launch_bounds__(kRcThreads) void rc_pick4_kernel(long long N, long long n, int n_tt, const int32_t* __restrict__ n_tt_dev,
                                                              int DP, int R, int step_r, int step_c, const int64_t* __restrict__ pos,
                                                              const float4* __restrict__ d_out, float4* __restrict__ d_rows) {
  rc_pick<float4>(N, n, n_tt, n_tt_dev, DP, R, step_r, step_c, pos, d_out, d_rows);
}

__global__ __launch_bounds__(kRcThreads) void rc_pick1_kernel(long long N, long long n, int n_tt, const int32_t* __restrict__ n_tt_dev,
                                                              int DP, int R, int step_r, int step_c, const int64_t* __restrict__ pos,
                                                              const float* __restrict__ d_out, float* __restrict__ d_rows) {
  rc_pick<float>(N, n, n_tt, n_tt_dev, DP, R, step_r, step_c, pos, d_out, d_rows);
}

static int rc_check_sizes(const char* what, int64_t N, int64_t n, int64_t n_tt, int32_t D) {
  if (N < 0 || n < 0 || n_tt < 0 || D <= 0 || N >= (1ll << 31))
    TTX_FAIL(TTX_EINVAL, "%s: bad N / n / n_tt / D (N=%lld, n=%lld, n_tt=%lld, D=%d)", what, (long long)N, (long long)n,
             (long long)n_tt, D);
  if (n > N) TTX_FAIL(TTX_EINVAL, "%s: n=%lld live lookups for N=%lld positions", what, (long long)n, (long long)N);
  if (n_tt > n) TTX_FAIL(TTX_EINVAL, "%s: n_tt=%lld misses among n=%lld live lookups", what, (long long)n_tt, (long long)n);
  return TTX_OK;
}

struct RcTile {
  bool v4;
  int DP, R, step_r, step_c;
  unsigned grid;
};

// `count` slots (an upper bound of the tiles' extent) of D floats
static RcTile rc_tile(int64_t count, int32_t D, bool v4) {
  RcTile t;
  t.v4 = v4;
  t.DP = v4 ? D / 4 : D;                               // pieces of a row
  t.R = t.DP >= kRcPieces ? 1 : kRcPieces / t.DP;      // slots of a tile
  t.step_r = kRcThreads / t.DP;
  t.step_c = kRcThreads % t.DP;
  const long long tiles = (count + t.R - 1) / t.R;
  // (a tile is one work-group: count < 2^31 tiles at most, the grid is capped and strides; offsets inside are 64-bit)
  t.grid = (unsigned)(tiles < kRcMaxBlocks ? tiles : kRcMaxBlocks);
  return t;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_rows_place(int64_t N, int64_t n, int64_t n_tt, const int32_t* n_tt_dev, int32_t D, const int64_t* pos, const int32_t* loc,
                   const float* rows_tt, const float* cache_weight, int64_t cache_size, const int64_t* rank, float* out,
                   ttx_stream_t stream) {
  const char* what = "rows_place";
  const int rc = rc_check_sizes(what, N, n, n_tt, D);
  if (rc) return rc;
  if (cache_size < 0 || cache_size >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: bad cache_size %lld", what, (long long)cache_size);
  if (!n_tt_dev && n_tt < n && cache_size <= 0)
    TTX_FAIL(TTX_EINVAL, "%s: %lld cached lookups and cache_size=%lld", what, (long long)(n - n_tt), (long long)cache_size);
  if (!rank && n != N)
    TTX_FAIL(TTX_EINVAL, "%s: without rank every position is live, got n=%lld for N=%lld", what, (long long)n, (long long)N);
  if ((((uintptr_t)rows_tt) | ((uintptr_t)cache_weight) | ((uintptr_t)out) | ((uintptr_t)loc) | ((uintptr_t)n_tt_dev)) & 3)
    TTX_FAIL(TTX_EINVAL, "%s: float / int32 pointers must be 4-byte aligned", what);
  if ((((uintptr_t)pos) | ((uintptr_t)rank)) & 7) TTX_FAIL(TTX_EINVAL, "%s: pos / rank must be 8-byte aligned", what);
  if (N == 0) return TTX_OK;
  if (!out) TTX_FAIL(TTX_EINVAL, "%s: NULL output", what);
  if (n > 0) {
    const bool any_tt = n_tt_dev || n_tt > 0, any_hit = n_tt_dev || n_tt < n;
    if (!pos || (any_tt && !rows_tt) || (any_hit && (!loc || !cache_weight))) TTX_FAIL(TTX_EINVAL, "%s: NULL input", what);
  }
  const bool v4 = D % 4 == 0 && ((((uintptr_t)rows_tt) | ((uintptr_t)cache_weight) | ((uintptr_t)out)) & 15) == 0;
  const RcTile t = rc_tile(N, D, v4);
  hipStream_t st = (hipStream_t)stream;
  if (v4)
    hipLaunchKernelGGL(rc_place4_kernel, dim3(t.grid), dim3(kRcThreads), 0, st, (long long)N, (long long)n, (int)n_tt, n_tt_dev, t.DP,
                       t.R, t.step_r, t.step_c, pos, loc, (const float4*)rows_tt, (const float4*)cache_weight, (long long)cache_size,
                       rank, (float4*)out);
  else
    hipLaunchKernelGGL(rc_place1_kernel, dim3(t.grid), dim3(kRcThreads), 0, st, (long long)N, (long long)n, (int)n_tt, n_tt_dev, t.DP,
                       t.R, t.step_r, t.step_c, pos, loc, rows_tt, cache_weight, (long long)cache_size, rank, out);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_rows_pick(int64_t N, int64_t n, int64_t n_tt, const int32_t* n_tt_dev, int32_t D, const int64_t* pos, const float* d_out,
                  float* d_rows, ttx_stream_t stream) {
  const char* what = "rows_pick";
  const int rc = rc_check_sizes(what, N, n, n_tt, D);
  if (rc) return rc;
  if ((((uintptr_t)d_out) | ((uintptr_t)d_rows) | ((uintptr_t)n_tt_dev)) & 3)
    TTX_FAIL(TTX_EINVAL, "%s: float / int32 pointers must be 4-byte aligned", what);
  if (((uintptr_t)pos) & 7) TTX_FAIL(TTX_EINVAL, "%s: pos must be 8-byte aligned", what);
  if (N == 0 || n == 0) return TTX_OK;
  if (!n_tt_dev && n_tt == 0) return TTX_OK;  // (nothing but hits: their gradient rows are read in place)
  if (!pos || !d_out || !d_rows) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  const bool v4 = D % 4 == 0 && ((((uintptr_t)d_out) | ((uintptr_t)d_rows)) & 15) == 0;
  const RcTile t = rc_tile(n_tt_dev ? n : n_tt, D, v4);
  hipStream_t st = (hipStream_t)stream;
  if (v4)
    hipLaunchKernelGGL(rc_pick4_kernel, dim3(t.grid), dim3(kRcThreads), 0, st, (long long)N, (long long)n, (int)n_tt, n_tt_dev, t.DP,
                       t.R, t.step_r, t.step_c, pos, (const float4*)d_out, (float4*)d_rows);
  else
    hipLaunchKernelGGL(rc_pick1_kernel, dim3(t.grid), dim3(kRcThreads), 0, st, (long long)N, (long long)n, (int)n_tt, n_tt_dev, t.DP,
                       t.R, t.step_r, t.step_c, pos, d_out, d_rows);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // extern "C"
