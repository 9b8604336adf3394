// ttx_cache_tables.hip -- the LFU row cache over SEVERAL tables of one table-batched bag (include/ttx.h, "row cache over
// several tables"; not in the reference, whose cache serves one table: tt_embeddings_ops.py:456).  gfx950, wave64.
//
// One hash table / frequency table / cache_state / cache_weight set serves all tables: a lookup (table t, index i) is the
// key t * key_stride + i.  Every cache kernel of ttx_cache.hip works on such keys and on bags addressed by their flat row
// t * B + b unchanged; this file carries (table, index) into key space (table_keys_kernel, counting the keys in the same
// launch), out of it again (table_keys_split_kernel: the misses of a partitioned batch, or the keys a populate selected) and
// decompresses the selected rows of any table (ttx_cache_populate_t).
#include "ttx_internal.h"

namespace ttx {

constexpr int kTK = 256;
constexpr int kTKStage = 1024;  // table boundaries (num_tables + 1 of them) staged in LDS up to here: 8 KiB

// keys[n] = indices[n] + t(n) * key_stride, t(n) = the table whose extent [offsets[t B], offsets[(t + 1) B]) holds n: the
// last of the num_tables + 1 boundaries that is <= n.  Empty tables give equal boundaries, which the search steps over; the
// closing boundary is nnz > n.  One thread per lookup; the boundaries come from LDS (staged != 0) or, beyond kTKStage of
// them, from the offsets themselves.  upd_hashtbl != NULL: update_cache_state (ttx_cache.hip) on the keys, same launch --
// every lane of a wave gets to hashtbl_count_wave (a wave-uniform call), so nothing returns early.
__global__ __launch_bounds__(kTK) void table_keys_kernel(int64_t N, const int64_t* __restrict__ indices, int32_t num_tables,
                                                        int64_t B, const int64_t* __restrict__ offsets, int64_t key_stride,
                                                        int64_t* __restrict__ keys, int32_t H, int64_t* upd_hashtbl,
                                                        int64_t* cache_freq, int32_t staged) {
  __shared__ int64_t tb[kTKStage];
  if (staged) {
    for (int i = threadIdx.x; i <= num_tables; i += kTK) tb[i] = offsets[(int64_t)i * B];
    __syncthreads();
  }
  const int64_t n = (int64_t)blockIdx.x * kTK + threadIdx.x;
  const bool valid = n < N;
  int64_t key = 0;
  if (valid) {
    int32_t lo = 1, hi = num_tables;  // the first boundary in [1, num_tables] that is > n (the closing one is)
    while (lo < hi) {
      const int32_t mid = (int32_t)(((int64_t)lo + hi) >> 1);
      const int64_t b = staged ? tb[mid] : offsets[(int64_t)mid * B];
      if (b > n) hi = mid;
      else lo = mid + 1;
    }
    key = indices[n] + (int64_t)(lo - 1) * key_stride;
    keys[n] = key;
  }
  if (upd_hashtbl) hashtbl_count_wave(key, valid, H, upd_hashtbl, cache_freq);
}

// The inverse on the first *n_dev entries (clamped to [0, n]; NULL: all n).  bagrow != NULL: entry s sits in bag
// bagrow[s] = t B + b of the flat batch -- the table comes from the bag (no 64-bit division), out_rowidx[s] = b.
// bagrow == NULL: t = keys[s] / key_stride (the keys a populate selected), out_rowidx is not written.  t is clamped to
// [0, num_tables - 1] before it scales anything; entries at and beyond the count are not written.
__global__ __launch_bounds__(kTK) void table_keys_split_kernel(int64_t n, const int32_t* __restrict__ n_dev, int32_t num_tables,
                                                              int64_t B, int64_t key_stride, const int64_t* __restrict__ keys,
                                                              const int64_t* __restrict__ bagrow, int64_t* __restrict__ out_idx,
                                                              int64_t* __restrict__ out_tab, int64_t* __restrict__ out_row) {
  int64_t cnt = n;
  if (n_dev) {
    const int64_t v = *n_dev;
    cnt = v < 0 ? 0 : (v < n ? v : n);
  }
  const int64_t s = (int64_t)blockIdx.x * kTK + threadIdx.x;
  if (s >= cnt) return;
  const int64_t k = keys[s];
  int64_t t;
  if (bagrow) {
    const int64_t r = bagrow[s];
    t = r / B;
    t = t < 0 ? 0 : (t < num_tables ? t : num_tables - 1);
    out_row[s] = r - t * B;
  } else {
    t = k / key_stride;
    t = t < 0 ? 0 : (t < num_tables ? t : num_tables - 1);
  }
  out_idx[s] = k - t * key_stride;
  out_tab[s] = t;
}

static int tk_check_sizes(const char* what, int64_t n, int32_t num_tables, int64_t B, int64_t key_stride) {
  if (n < 0 || n >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: %lld lookups out of range [0, 2^31)", what, (long long)n);
  if (num_tables <= 0 || B <= 0 || key_stride <= 0)
    TTX_FAIL(TTX_EINVAL, "%s: num_tables=%d, B=%lld and key_stride=%lld must be > 0", what, num_tables, (long long)B,
             (long long)key_stride);
  if (B >= (1ll << 31) || (int64_t)num_tables * B >= (1ll << 31))
    TTX_FAIL(TTX_EINVAL, "%s: %d tables of %lld bags: the batch must hold fewer than 2^31 bags", what, num_tables, (long long)B);
  if (key_stride >= (1ll << 62) / num_tables)
    TTX_FAIL(TTX_EINVAL, "%s: the key space num_tables * key_stride = %d * %lld must stay below 2^62", what, num_tables,
             (long long)key_stride);
  return TTX_OK;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_table_keys(int64_t nnz, const int64_t* indices, int32_t num_tables, int64_t B, const int64_t* offsets,
                   int64_t key_stride, int64_t* keys, int64_t H, int64_t* upd_hashtbl, int64_t* upd_cache_freq,
                   ttx_stream_t stream) {
  const char* what = "table_keys";
  const int rc = tk_check_sizes(what, nnz, num_tables, B, key_stride);
  if (rc) return rc;
  const bool upd = upd_hashtbl || upd_cache_freq;
  if (upd && (!upd_hashtbl || !upd_cache_freq)) TTX_FAIL(TTX_EINVAL, "%s: counting needs both hashtbl and cache_freq", what);
  if (upd && (H <= 0 || H >= (1ll << 31))) TTX_FAIL(TTX_EINVAL, "%s: hashtbl_size=%lld must be in (0, 2^31)", what, (long long)H);
  if ((((uintptr_t)indices) | ((uintptr_t)offsets) | ((uintptr_t)keys) | ((uintptr_t)upd_hashtbl) | ((uintptr_t)upd_cache_freq)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: int64 pointers must be 8-byte aligned", what);
  if (nnz == 0) return TTX_OK;
  if (!indices || !offsets || !keys) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  hipLaunchKernelGGL(table_keys_kernel, dim3((unsigned)((nnz + kTK - 1) / kTK)), dim3(kTK), 0, (hipStream_t)stream, nnz, indices,
                     num_tables, B, offsets, key_stride, keys, (int32_t)(upd ? H : 0), upd_hashtbl, upd_cache_freq,
                     (int32_t)(num_tables + 1 <= kTKStage));
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_table_keys_split(int64_t n, const int32_t* n_dev, int32_t num_tables, int64_t B, int64_t key_stride, const int64_t* keys,
                         const int64_t* bagrow, int64_t* out_indices, int64_t* out_tableidx, int64_t* out_rowidx,
                         ttx_stream_t stream) {
  const char* what = "table_keys_split";
  const int rc = tk_check_sizes(what, n, num_tables, B, key_stride);
  if (rc) return rc;
  if (((uintptr_t)n_dev) & 3) TTX_FAIL(TTX_EINVAL, "%s: n_dev must be 4-byte aligned", what);
  if ((((uintptr_t)keys) | ((uintptr_t)bagrow) | ((uintptr_t)out_indices) | ((uintptr_t)out_tableidx) | ((uintptr_t)out_rowidx)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: int64 pointers must be 8-byte aligned", what);
  if (n == 0) return TTX_OK;
  if (!keys || !out_indices || !out_tableidx || (bagrow && !out_rowidx)) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  hipLaunchKernelGGL(table_keys_split_kernel, dim3((unsigned)((n + kTK - 1) / kTK)), dim3(kTK), 0, (hipStream_t)stream, n, n_dev,
                     num_tables, B, key_stride, keys, bagrow, out_indices, out_tableidx, out_rowidx);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

// workspace: [the sort's | cache_size indices | cache_size tables | the plan of the cache_size rows]
size_t ttx_cache_populate_t_workspace_bytes(const ttx_geom* g, int64_t H, int64_t cache_size, int32_t D) {
  (void)D;
  Dims d;
  if (!g || g->p_tables || make_dims(g, &d) != TTX_OK || H <= 0 || cache_size < 0) return 0;
  return populate_sort_ws_bytes(H) + 2 * align_up((size_t)cache_size * 8) + plan_bytes(d, cache_size) + 256;
}

int ttx_cache_populate_t(const ttx_geom* g, const float* const* tt_cores, int64_t H, int64_t* hashtbl, int64_t* cache_freq,
                         int32_t* cache_state, int64_t cache_size, int32_t D, float* cache_weight, int64_t key_stride,
                         int32_t flags, void* workspace, size_t workspace_bytes, ttx_stream_t stream) {
  const char* what = "cache_populate_t";
  if (flags & ~TTX_POPULATE_REFERENCE_EXACT) TTX_FAIL(TTX_EINVAL, "%s: unknown flags %d", what, flags);
  if (!g) TTX_FAIL(TTX_EINVAL, "%s: NULL geometry", what);
  if (g->p_tables) TTX_FAIL(TTX_EINVAL, "%s: tables of one row shape only (no p_tables)", what);
  if (g->num_tables <= 0 || key_stride <= 0)
    TTX_FAIL(TTX_EINVAL, "%s: num_tables=%d and key_stride=%lld must be > 0", what, g->num_tables, (long long)key_stride);
  if (key_stride >= (1ll << 62) / g->num_tables)
    TTX_FAIL(TTX_EINVAL, "%s: the key space num_tables * key_stride = %d * %lld must stay below 2^62", what, g->num_tables,
             (long long)key_stride);
  if (H <= 0 || H >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: hashtbl_size=%lld must be in (0, 2^31)", what, (long long)H);
  if (cache_size < 0 || cache_size > H) TTX_FAIL(TTX_EINVAL, "%s: cache_size=%lld must be in [0, hashtbl_size]", what, (long long)cache_size);
  if (D <= 0) TTX_FAIL(TTX_EINVAL, "%s: D=%d must be > 0", what, D);
  if ((((uintptr_t)hashtbl) | ((uintptr_t)cache_freq) | ((uintptr_t)workspace)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: hashtbl / cache_freq / workspace must be 8-byte aligned", what);
  if ((((uintptr_t)cache_state) | ((uintptr_t)cache_weight)) & 3)
    TTX_FAIL(TTX_EINVAL, "%s: cache_state / cache_weight must be 4-byte aligned", what);
  if (!hashtbl || !cache_freq || !cache_state || !tt_cores) TTX_FAIL(TTX_EINVAL, "%s: NULL input", what);
  if (cache_size > 0 && !cache_weight) TTX_FAIL(TTX_EINVAL, "%s: cache_weight is NULL", what);
  Dims d;
  int rc = make_dims(g, &d);
  if (rc) return rc;
  long long rows = 1;  // the range the index decode covers: an index below key_stride must lie inside it
  for (int t = 0; t < d.T; ++t) rows *= d.p[t];
  if (key_stride > rows)
    TTX_FAIL(TTX_EINVAL, "%s: key_stride=%lld exceeds the tables' prod(p)=%lld rows", what, (long long)key_stride, rows);
  if (!workspace || workspace_bytes < ttx_cache_populate_t_workspace_bytes(g, H, cache_size, D))
    TTX_FAIL(TTX_EWORKSPACE, "%s: workspace too small", what);
  hipStream_t st = (hipStream_t)stream;
  char* ws = (char*)workspace;
  int64_t* sorted_keys = nullptr;
  rc = populate_sort_mark(H, hashtbl, cache_freq, cache_state, cache_size, flags & TTX_POPULATE_REFERENCE_EXACT, ws, &sorted_keys, st);
  if (rc) return rc;
  if (cache_size == 0) return TTX_OK;
  int64_t* idx = (int64_t*)(ws + populate_sort_ws_bytes(H));
  int64_t* tab = (int64_t*)((char*)idx + align_up((size_t)cache_size * 8));
  char* rows_ws = (char*)tab + align_up((size_t)cache_size * 8);
  // (an empty slot among the first cache_size was made key 0 by the mark: row 0 of table 0)
  rc = ttx_table_keys_split(cache_size, nullptr, d.num_tables, 1, key_stride, sorted_keys, nullptr, idx, tab, nullptr, stream);
  if (rc) return rc;
  return ttx_tt_rows(g, D, cache_size, idx, tab, tt_cores, cache_weight, rows_ws, plan_bytes(d, cache_size), stream);
}

}  // extern "C"
