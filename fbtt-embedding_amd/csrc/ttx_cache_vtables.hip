// ttx_cache_vtables.hip -- the LFU row cache over the tables of DIFFERENT row factors of one batched bag (include/ttx.h, "row
// cache over tables of different row factors"; ttx_geom::p_tables).  gfx950, wave64.
//
// ttx_cache_tables.hip keys a lookup (table t, index i) by t * key_stride + i: one stride, because its tables have one row
// shape.  Here table k covers stride_k = prod_t p_tables[k][t] rows and its keys are key_base[k] + i, key_base[k] = the sum of
// the strides in front of it, key_base[num_tables] = the total.  The ranges are disjoint (i < num_embeddings_k <= stride_k),
// every cache kernel of ttx_cache.hip works on such keys unchanged, and this file carries (table, index) into key space
// (table_keys_v_kernel, counting the keys in the same launch), out of it again (table_keys_split_v_kernel) and decompresses
// the rows a populate selected, each from its own table (ttx_cache_populate_v).
//
// key_base is a HOST array read during the call: it travels by value in the kernel arguments (65 int64: no device
// allocation, no copy from pageable memory, capturable) and is staged in LDS through constant subscripts -- a run-time
// subscript into the by-value struct would send it through scratch memory (ttx_internal.h TTX_PICK_BATCH).
#include "ttx_internal.h"

namespace ttx {

constexpr int kVK = 256;
constexpr int kVKBases = TTX_MAX_TABLES_MIXED + 1;
static_assert(kVKBases <= kVK, "one thread stages one key base");

struct KeyBases {
  int64_t v[kVKBases];  // entries beyond num_tables repeat the total
};

// sb[k] = kb.v[k], k < kVKBases: thread k picks its entry with constant subscripts (65 selects on scalar operands)
__device__ __forceinline__ void stage_key_bases(const KeyBases& kb, int64_t* sb) {
  const int tid = threadIdx.x;
  int64_t v = 0;
#pragma unroll
  for (int k = 0; k < kVKBases; ++k) v = tid == k ? kb.v[k] : v;
  if (tid < kVKBases) sb[tid] = v;
}

// keys[n] = indices[n] + key_base[t(n)], t(n) found as table_keys_kernel (ttx_cache_tables.hip) finds it: the last of the
// num_tables + 1 table boundaries offsets[t B] that is <= n.  Empty tables give equal boundaries, which the search steps
// over; the closing boundary is nnz > n.  One thread per lookup, boundaries and bases from LDS.  upd_hashtbl != NULL: the keys
// are counted in the same launch -- every lane of a wave gets to hashtbl_count_wave (a wave-uniform call): nothing returns early.
__global__ __launch_bounds__(kVK) void table_keys_v_kernel(int64_t N, const int64_t* __restrict__ indices, int32_t num_tables,
                                                          int64_t B, const int64_t* __restrict__ offsets, const KeyBases kb,
                                                          int64_t* __restrict__ keys, int32_t H, int64_t* upd_hashtbl,
                                                          int64_t* cache_freq) {
  __shared__ int64_t tb[kVKBases];
  __shared__ int64_t sb[kVKBases];
  stage_key_bases(kb, sb);
  if ((int)threadIdx.x <= num_tables) tb[threadIdx.x] = offsets[(int64_t)threadIdx.x * B];
  __syncthreads();
  const int64_t n = (int64_t)blockIdx.x * kVK + threadIdx.x;
  const bool valid = n < N;
  int64_t key = 0;
  if (valid) {
    int32_t lo = 1, hi = num_tables;  // the first boundary in [1, num_tables] that is > n (the closing one is)
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (tb[mid] > n) hi = mid;
      else lo = mid + 1;
    }
    key = indices[n] + sb[lo - 1];
    keys[n] = key;
  }
  if (upd_hashtbl) hashtbl_count_wave(key, valid, H, upd_hashtbl, cache_freq);
}

// The inverse on the first *n_dev entries (clamped to [0, n]; NULL: all n).  bagrow != NULL: entry s sits in bag
// bagrow[s] = t B + b of the flat batch, out_rowidx[s] = b.  bagrow == NULL (the keys a populate selected): t = the last k in
// [0, num_tables - 1] with key_base[k] <= key, at most 6 steps over the staged bases (tables of stride 1 are found like any
// other: their bases differ by 1); out_rowidx is not written.  t is clamped to [0, num_tables - 1] before it indexes
// anything; entries at and beyond the count are not written.
__global__ __launch_bounds__(kVK) void table_keys_split_v_kernel(int64_t n, const int32_t* __restrict__ n_dev, int32_t num_tables,
                                                                int64_t B, const KeyBases kb, const int64_t* __restrict__ keys,
                                                                const int64_t* __restrict__ bagrow, int64_t* __restrict__ out_idx,
                                                                int64_t* __restrict__ out_tab, int64_t* __restrict__ out_row) {
  __shared__ int64_t sb[kVKBases];
  stage_key_bases(kb, sb);
  __syncthreads();
  int64_t cnt = n;
  if (n_dev) {
    const int64_t v = *n_dev;
    cnt = v < 0 ? 0 : (v < n ? v : n);
  }
  const int64_t s = (int64_t)blockIdx.x * kVK + threadIdx.x;
  if (s >= cnt) return;
  const int64_t k = keys[s];
  int32_t t;
  if (bagrow) {
    const int64_t r = bagrow[s];
    const int64_t tr = r / B;
    t = tr < 0 ? 0 : (tr < num_tables ? (int32_t)tr : num_tables - 1);
    out_row[s] = r - (int64_t)t * B;
  } else {
    int32_t lo = 0, hi = num_tables - 1;
    while (lo < hi) {
      const int32_t mid = (lo + hi + 1) >> 1;
      if (sb[mid] <= k) lo = mid;
      else hi = mid - 1;
    }
    t = lo;
  }
  out_idx[s] = k - sb[t];
  out_tab[s] = t;
}

// sizes and the key bases (host memory, num_tables + 1 entries): -> kb, padded with the total
static int vk_check(const char* what, int64_t n, int32_t num_tables, int64_t B, const int64_t* key_base, KeyBases* kb) {
  if (n < 0 || n >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: %lld lookups out of range [0, 2^31)", what, (long long)n);
  if (num_tables < 1 || num_tables > TTX_MAX_TABLES_MIXED)
    TTX_FAIL(TTX_EINVAL, "%s: num_tables=%d must be in [1, %d]", what, num_tables, TTX_MAX_TABLES_MIXED);
  if (B <= 0) TTX_FAIL(TTX_EINVAL, "%s: B=%lld must be > 0", what, (long long)B);
  if (B >= (1ll << 31) || (int64_t)num_tables * B >= (1ll << 31))
    TTX_FAIL(TTX_EINVAL, "%s: %d tables of %lld bags: the batch must hold fewer than 2^31 bags", what, num_tables, (long long)B);
  if (!key_base) TTX_FAIL(TTX_EINVAL, "%s: key_base is NULL", what);
  if (((uintptr_t)key_base) & 7) TTX_FAIL(TTX_EINVAL, "%s: key_base must be 8-byte aligned", what);
  if (key_base[0] != 0) TTX_FAIL(TTX_EINVAL, "%s: key_base[0]=%lld must be 0", what, (long long)key_base[0]);
  for (int k = 0; k < num_tables; ++k)
    if (key_base[k + 1] <= key_base[k])
      TTX_FAIL(TTX_EINVAL, "%s: key_base must be strictly increasing (entries %d, %d: %lld, %lld)", what, k, k + 1,
               (long long)key_base[k], (long long)key_base[k + 1]);
  if (key_base[num_tables] >= (1ll << 62))
    TTX_FAIL(TTX_EINVAL, "%s: the key space key_base[num_tables]=%lld must stay below 2^62", what, (long long)key_base[num_tables]);
  for (int k = 0; k < kVKBases; ++k) kb->v[k] = key_base[k < num_tables ? k : num_tables];
  return TTX_OK;
}

// key_base of a p_tables geometry: the running sum of the tables' prod(p)
static int vk_bases_of(const char* what, const ttx_geom* g, int64_t* key_base) {
  key_base[0] = 0;
  for (int k = 0; k < g->num_tables; ++k) {
    int64_t rows = 1;
    for (int t = 0; t < g->T; ++t) {
      const int pk = g->p_tables[(size_t)k * g->T + t];
      if (pk <= 0) TTX_FAIL(TTX_EINVAL, "%s: table %d core %d: p must be > 0", what, k, t);
      if (rows > (1ll << 62) / pk) TTX_FAIL(TTX_EINVAL, "%s: table %d: prod(p) does not fit the key space of 2^62", what, k);
      rows *= pk;
    }
    if (rows >= (1ll << 62) - key_base[k]) TTX_FAIL(TTX_EINVAL, "%s: the key space sum prod(p_tables) must stay below 2^62", what);
    key_base[k + 1] = key_base[k] + rows;
  }
  return TTX_OK;
}

}  // namespace ttx

using namespace ttx;

extern "C" {

int ttx_table_keys_v(int64_t nnz, const int64_t* indices, int32_t num_tables, int64_t B, const int64_t* offsets,
                     const int64_t* key_base, int64_t* keys, int64_t H, int64_t* upd_hashtbl, int64_t* upd_cache_freq,
                     ttx_stream_t stream) {
  const char* what = "table_keys_v";
  KeyBases kb;
  const int rc = vk_check(what, nnz, num_tables, B, key_base, &kb);
  if (rc) return rc;
  const bool upd = upd_hashtbl || upd_cache_freq;
  if (upd && (!upd_hashtbl || !upd_cache_freq)) TTX_FAIL(TTX_EINVAL, "%s: counting needs both hashtbl and cache_freq", what);
  if (upd && (H <= 0 || H >= (1ll << 31))) TTX_FAIL(TTX_EINVAL, "%s: hashtbl_size=%lld must be in (0, 2^31)", what, (long long)H);
  if ((((uintptr_t)indices) | ((uintptr_t)offsets) | ((uintptr_t)keys) | ((uintptr_t)upd_hashtbl) | ((uintptr_t)upd_cache_freq)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: int64 pointers must be 8-byte aligned", what);
  if (nnz == 0) return TTX_OK;
  if (!indices || !offsets || !keys) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  hipLaunchKernelGGL(table_keys_v_kernel, dim3((unsigned)((nnz + kVK - 1) / kVK)), dim3(kVK), 0, (hipStream_t)stream, nnz, indices,
                     num_tables, B, offsets, kb, keys, (int32_t)(upd ? H : 0), upd_hashtbl, upd_cache_freq);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

int ttx_table_keys_split_v(int64_t n, const int32_t* n_dev, int32_t num_tables, int64_t B, const int64_t* key_base,
                           const int64_t* keys, const int64_t* bagrow, int64_t* out_indices, int64_t* out_tableidx,
                           int64_t* out_rowidx, ttx_stream_t stream) {
  const char* what = "table_keys_split_v";
  KeyBases kb;
  const int rc = vk_check(what, n, num_tables, B, key_base, &kb);
  if (rc) return rc;
  if (((uintptr_t)n_dev) & 3) TTX_FAIL(TTX_EINVAL, "%s: n_dev must be 4-byte aligned", what);
  if ((((uintptr_t)keys) | ((uintptr_t)bagrow) | ((uintptr_t)out_indices) | ((uintptr_t)out_tableidx) | ((uintptr_t)out_rowidx)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: int64 pointers must be 8-byte aligned", what);
  if (n == 0) return TTX_OK;
  if (!keys || !out_indices || !out_tableidx || (bagrow && !out_rowidx)) TTX_FAIL(TTX_EINVAL, "%s: NULL input / output", what);
  hipLaunchKernelGGL(table_keys_split_v_kernel, dim3((unsigned)((n + kVK - 1) / kVK)), dim3(kVK), 0, (hipStream_t)stream, n, n_dev,
                     num_tables, B, kb, keys, bagrow, out_indices, out_tableidx, out_rowidx);
  TTX_HIP(hipGetLastError());
  return TTX_OK;
}

// workspace: [the sort's | cache_size indices | cache_size tables | the plan of the cache_size rows]
size_t ttx_cache_populate_v_workspace_bytes(const ttx_geom* g, int64_t H, int64_t cache_size, int32_t D) {
  (void)D;
  Dims d;
  if (!g || !g->p_tables || g->T != 3 || H <= 0 || cache_size < 0 || make_dims(g, &d) != TTX_OK) return 0;
  return populate_sort_ws_bytes(H) + 2 * align_up((size_t)cache_size * 8) + plan_bytes(d, cache_size) + 256;
}

int ttx_cache_populate_v(const ttx_geom* g, const float* const* tt_cores, int64_t H, int64_t* hashtbl, int64_t* cache_freq,
                         int32_t* cache_state, int64_t cache_size, int32_t D, float* cache_weight, int32_t flags, void* workspace,
                         size_t workspace_bytes, ttx_stream_t stream) {
  const char* what = "cache_populate_v";
  if (flags & ~TTX_POPULATE_REFERENCE_EXACT) TTX_FAIL(TTX_EINVAL, "%s: unknown flags %d", what, flags);
  if (!g) TTX_FAIL(TTX_EINVAL, "%s: NULL geometry", what);
  if (!g->p_tables) TTX_FAIL(TTX_EINVAL, "%s: the geometry must carry per-table row factors (p_tables)", what);
  if (g->num_tables < 1 || g->num_tables > TTX_MAX_TABLES_MIXED)
    TTX_FAIL(TTX_EINVAL, "%s: num_tables=%d must be in [1, %d]", what, g->num_tables, TTX_MAX_TABLES_MIXED);
  if (g->T < 2 || g->T > TTX_MAX_CORES) TTX_FAIL(TTX_EINVAL, "%s: T=%d: number of TT cores must be 2..4", what, g->T);
  // (the rows route on a plan with per-table row factors has only ever run with three cores)
  if (g->T != 3) TTX_FAIL(TTX_EUNSUPPORTED, "%s: tables of different row factors are populated with three TT cores only (T=%d)", what, g->T);
  int64_t key_base[kVKBases];
  int rc = vk_bases_of(what, g, key_base);
  if (rc) return rc;
  if (H <= 0 || H >= (1ll << 31)) TTX_FAIL(TTX_EINVAL, "%s: hashtbl_size=%lld must be in (0, 2^31)", what, (long long)H);
  if (cache_size < 0 || cache_size > H) TTX_FAIL(TTX_EINVAL, "%s: cache_size=%lld must be in [0, hashtbl_size]", what, (long long)cache_size);
  if (D <= 0) TTX_FAIL(TTX_EINVAL, "%s: D=%d must be > 0", what, D);
  if ((((uintptr_t)hashtbl) | ((uintptr_t)cache_freq) | ((uintptr_t)workspace)) & 7)
    TTX_FAIL(TTX_EINVAL, "%s: hashtbl / cache_freq / workspace must be 8-byte aligned", what);
  if ((((uintptr_t)cache_state) | ((uintptr_t)cache_weight)) & 3)
    TTX_FAIL(TTX_EINVAL, "%s: cache_state / cache_weight must be 4-byte aligned", what);
  if (!hashtbl || !cache_freq || !cache_state || !tt_cores) TTX_FAIL(TTX_EINVAL, "%s: NULL input", what);
  if (cache_size > 0 && !cache_weight) TTX_FAIL(TTX_EINVAL, "%s: cache_weight is NULL", what);
  Dims d;  // (from here on a device may be touched: a geometry seen for the first time places its per-table factors there)
  rc = make_dims(g, &d);
  if (rc) return rc;
  const size_t rows_bytes = plan_bytes(d, cache_size);
  if (!workspace || workspace_bytes < populate_sort_ws_bytes(H) + 2 * align_up((size_t)cache_size * 8) + rows_bytes + 256)
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
  rc = ttx_table_keys_split_v(cache_size, nullptr, d.num_tables, 1, key_base, sorted_keys, nullptr, idx, tab, nullptr, stream);
  if (rc) return rc;
  return ttx_tt_rows(g, D, cache_size, idx, tab, tt_cores, cache_weight, rows_ws, rows_bytes, stream);
}

}  // extern "C"
