// ttx_rows.hip -- compacted rows <-> positions of a padded unpooled lookup (nn.Embedding's padding_idx; not in the reference).
//
// ttx_bags_compact over n bags of ONE slot leaves rank[i] = live positions in front of position i (n + 1 entries); position i
// is live iff rank[i + 1] > rank[i], and its row is row rank[i] of the compacted batch.  ttx_rows_expand puts the rows of the
// compacted lookup back at their positions and writes exact zeros at the padding (every element of `out` has one writer: no
// memset in front); ttx_rows_collect is its transpose, the gradient rows of the live positions in compacted order (rows at
// and beyond rank[n] are left alone: the plan's live count keeps every later kernel away from them).
//
// Both move bytes and nothing else.  A work-group takes a tile of R consecutive positions -- R chosen so that a tile holds
// about kRowsPieces pieces, short rows (D = 12 .. 64) grouped so that they still fill the waves -- and its threads walk the
// tile's pieces in order: a piece is 16 bytes (float4: D % 4 == 0 and all three float pointers 16-byte aligned) or one float
// (anything else), consecutive lanes hold consecutive pieces of `out` / `d_out`, kRowsUnroll pieces per thread in flight.  The
// (position, column) of a thread's next piece follows from the last one by an add and a compare (the tile's stride 256 =
// step_r * DP + step_c on the host): no division in the loop.  Element offsets are 64-bit (n * D * 4 may pass 2^32).  No
// atomics, no LDS, no workspace, nothing read back: bit-identical from run to run, capturable.
#include "ttx_internal.h"

namespace ttx {

constexpr int kRowsThreads = 256;
constexpr int kRowsUnroll = 4;
constexpr int kRowsPieces = kRowsThreads * kRowsUnroll;  // pieces of a tile of short rows
constexpr long long kRowsMaxBlocks = 1ll << 20;          // grid.x (tiles beyond it: the work-groups stride over them)

// rank[i] clamped to the n rows there are; live = rank[i + 1] > rank[i]
__device__ __forceinline__ long long rows_rank(const int64_t* __restrict__ rank, long long i, long long n, bool* live) {
  const long long a = rank[i], b = rank[i + 1];
  *live = b > a;
  return a < 0 ? 0 : (a > n - 1 ? n - 1 : a);
}

// EXPAND: dense = out [n, DP] pieces, packed = rows;  else: dense = d_out, packed = d_rows
template <typename V, bool EXPAND>
__device__ __forceinline__ void rows_move(long long n, int DP, int R, int step_r, int step_c, const int64_t* __restrict__ rank,
                                          const V* __restrict__ src, V* __restrict__ dst) {
  const long long tiles = (n + R - 1) / R;
  const unsigned tid = threadIdx.x;
  const int r_first = (int)(tid / (unsigned)DP), c_first = (int)(tid - (unsigned)r_first * (unsigned)DP);
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long i0 = tile * R;
    const int rows_here = (int)(n - i0 < R ? n - i0 : R);
    int r = r_first, c = c_first;
    while (r < rows_here) {
      V v[kRowsUnroll];
      long long at[kRowsUnroll];  // piece offset of the store, -1: none
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u) {
        at[u] = -1;
        v[u] = V{};  // (every element assigned on every path: the arrays stay in registers)
        if (r < rows_here) {
          const long long i = i0 + r;
          bool live;
          const long long k = rows_rank(rank, i, n, &live);
          if constexpr (EXPAND) {
            at[u] = i * DP + c;
            if (live) v[u] = src[k * DP + c];
          } else if (live) {
            at[u] = k * DP + c;
            v[u] = src[i * DP + c];
          }
        }
        r += step_r;
        c += step_c;
        if (c >= DP) { c -= DP; ++r; }
      }
#pragma unroll
      for (int u = 0; u < kRowsUnroll; ++u)
        if (at[u] >= 0) dst[at[u]] = v[u];
    }
  }
}

__global__ __launch_bounds__(kRowsThreads) void rows_expand4_kernel(long long n, int DP, int R, int step_r, int step_c,
                                                                    const int64_t* __restrict__ rank,
                                                                    const float4* __restrict__ rows, float4* __restrict__ out) {
  rows_move<float4, true>(n, DP, R, step_r, step_c, rank, rows, out);
}

__global__ __launch_bounds__(kRowsThreads) void rows_expand1_kernel(long long n, int DP, int R, int step_r, int step_c,
                                                                    const int64_t* __restrict__ rank,
                                                                    const float* __restrict__ rows, float* __restrict__ out) {
  rows_move<float, true>(n, DP, R, step_r, step_c, rank, rows, out);
}

__global__ __launch_bounds__(kRowsThreads) void rows_collect4_kernel(long long n, int DP, int R, int step_r, int step_c,
                                                                     const int64_t* __restrict__ rank,
                                                                     const float4* __restrict__ d_out, float4* __restrict__ d_rows) {
  rows_move<float4, false>(n, DP, R, step_r, step_c, rank, d_out, d_rows);
}

__global__ __launch_bounds__(kRowsThreads) void rows_collect1_kernel(long long n, int DP, int R, int step_r, int step_c,
                                                                     const int64_t* __restrict__ rank,
                                                                     const float* __restrict__ d_out, float* __restrict__ d_rows) {
  rows_move<float, false>(n, DP, R, step_r, step_c, rank, d_out, d_rows);
}

static int rows_check(const char* what, int64_t n, int32_t D, const int64_t* rank, const float* a, const float* b) {
  if (n < 0 || D <= 0 || n >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: bad n / D (n=%lld, D=%d)", what, (long long)n, D);
  if (((uintptr_t)a | (uintptr_t)b) & 3) TTX_FAIL(TTX_EINVAL, "%s: float pointers must be 4-byte aligned", what);
  if (((uintptr_t)rank) & 7) TTX_FAIL(TTX_EINVAL, "%s: rank must be 8-byte aligned", what);
  if (n > 0 && (!rank || !a || !b)) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  return TTX_OK;
}

template <bool EXPAND>
static int rows_launch(int64_t n, int32_t D, const int64_t* rank, const float* src, float* dst, hipStream_t st) {
  const bool v4 = D % 4 == 0 && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
  const int DP = v4 ? D / 4 : D;                           // pieces of a row
  const int R = DP >= kRowsPieces ? 1 : kRowsPieces / DP;  // positions of a tile
  const int step_r = kRowsThreads / DP, step_c = kRowsThreads % DP;
  const long long tiles = (n + R - 1) / R;
  // (a tile is one work-group: n < 2^31 tiles at most, the grid is capped and strides; offsets inside are 64-bit)
  const unsigned grid = (unsigned)(tiles < kRowsMaxBlocks ? tiles : kRowsMaxBlocks);
  if (v4) {
    if (EXPAND)
      hipLaunchKernelGGL(rows_expand4_kernel, dim3(grid), dim3(kRowsThreads), 0, st, (long long)n, DP, R, step_r, step_c, rank,
                         (const float4*)src, (float4*)dst);
    else
      hipLaunchKernelGGL(rows_collect4_kernel, dim3(grid), dim3(kRowsThreads), 0, st, (long long)n, DP, R, step_r, step_c, rank,
                         (const float4*)src, (float4*)dst);
  } else {
    if (EXPAND)
      hipLaunchKernelGGL(rows_expand1_kernel, dim3(grid), dim3(kRowsThreads), 0, st, (long long)n, DP, R, step_r, step_c, rank, src,
                         dst);
    else
      hipLaunchKernelGGL(rows_collect1_kernel, dim3(grid), dim3(kRowsThreads), 0, st, (long long)n, DP, R, step_r, step_c, rank, src,
                         dst);
  }
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_rows_expand(int64_t n, int32_t D, const int64_t* rank, const float* rows, float* out, ttx_stream_t stream) {
  const int rc = rows_check("rows_expand", n, D, rank, rows, out);
  if (rc) return rc;
  if (n == 0) return TTX_OK;
  return rows_launch<true>(n, D, rank, rows, out, (hipStream_t)stream);
}

int ttx_rows_collect(int64_t n, int32_t D, const int64_t* rank, const float* d_out, float* d_rows, ttx_stream_t stream) {
  const int rc = rows_check("rows_collect", n, D, rank, d_out, d_rows);
  if (rc) return rc;
  if (n == 0) return TTX_OK;
  return rows_launch<false>(n, D, rank, d_out, d_rows, (hipStream_t)stream);
}

}  // extern "C"
