/*
 * ttx.h -- C ABI of libttx.so: MI355X (gfx950) native TT-compressed EmbeddingBag.
 *
 * This header is the drop-in boundary for the hot path of
 * facebookresearch/FBTT-Embedding.  Every entry point below replaces one of the
 * eleven functions the reference exports from its native module `tt_embeddings`
 * (reference tt_embeddings.cpp:131-161); the reference prototype each one
 * replaces is cited next to it.  Signatures carry only plain pointers, sizes and
 * scalars (no torch / ATen types): the Python shim
 * fbtt-embedding_amd/tt_embeddings.py binds them with ctypes, and INTEGRATION.md
 * shows the pybind11 stub a maintainer of the reference would write instead.
 *
 * Conventions
 *  - All data pointers are DEVICE pointers (HBM) unless the name ends in _host.
 *    `tt_cores`, `optimizer_state`, `d_tt_cores` are HOST arrays of T device
 *    pointers (one per TT core).
 *  - Index tensors are int64 (as in the reference), cores/outputs fp32, all
 *    contiguous.  Core t has shape [num_tables, p[t], r[t]*q[t]*r[t+1]]; each
 *    p-slice is row-major [r[t]][q[t]][r[t+1]] (reference tt_embeddings_ops.py
 *    :513-530, :601-611).
 *  - `stream` is a hipStream_t.  All work is enqueued on it; nothing
 *    synchronises with the host except ttx_preprocess_indices_sync in the
 *    cache-live case (exactly like the reference, tt_embeddings_cuda.cu:1481-1488)
 *    and ttx_cache_populate (one 8-byte read-back to size the radix sort).
 *  - `workspace` is caller-provided device scratch of at least the size the
 *    matching *_workspace_bytes() query returns (256-byte aligned).  No entry
 *    point allocates device memory.
 *  - Return value: 0 on success, negative TTX_E* on error;
 *    ttx_last_error() returns a thread-local message for the last failure.
 *  - Strides L[t] = prod_{s>t} p[s] (reference tt_embeddings_ops.py:506-512) are
 *    derived from `p` on the host; the reference's device tensor `L` is not read.
 */
#ifndef TTX_H_
#define TTX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTX_MAX_CORES 4

#define TTX_OK 0
#define TTX_EINVAL (-1)    /* bad argument (mirrors the reference's TORCH_CHECKs) */
#define TTX_EWORKSPACE (-2) /* workspace too small */
#define TTX_EUNSUPPORTED (-3) /* geometry does not fit this build's LDS tiling */
#define TTX_EHIP (-4)       /* a HIP runtime call failed */

/* fused-optimizer selector of ttx_tt_backward (reference OPTIM_* enum,
 * tt_embeddings_cuda.cu:31-35) */
#define TTX_OPTIM_SGD 0
#define TTX_OPTIM_ADAGRAD 1
#define TTX_OPTIM_DENSE 2

typedef void* ttx_stream_t; /* hipStream_t */

#define TTX_MAX_TABLES_MIXED 64

/* TT geometry shared by all tables of one TableBatchedTTEmbeddingBag
 * (reference tt_embeddings_ops.py:459-488).
 *
 * p_tables (beyond the reference, which batches tables of ONE shape only,
 * tt_embeddings_ops.py:424): NULL, or a host array [num_tables][T] of per-table
 * row factors -- tables of different cardinality in one batched lookup
 * (num_tables <= TTX_MAX_TABLES_MIXED).  q and the ranks stay common, so every core
 * slice has one size and core t is ONE array of sum_k p_tables[k][t] slices, table
 * after table: tt_cores[t] points at [sum_k p_k_t][r_t q_t r_{t+1}] floats and the
 * slice of (table k, i_t) is base_t[k] + i_t with base_t[k] = sum_{j<k} p_tables[j][t].
 * p[] is ignored then.  Only the calls that take tableidx accept such a geometry (plan,
 * forward, backward; not the one-table cache entry points).  The array is read during
 * the call only. */
typedef struct ttx_geom {
  int32_t T;                    /* number of TT cores, 2..4 */
  int32_t num_tables;           /* tt_cores[t].size(0) */
  int32_t p[TTX_MAX_CORES];     /* tt_p_shapes */
  int32_t q[TTX_MAX_CORES];     /* tt_q_shapes */
  int32_t r[TTX_MAX_CORES + 1]; /* padded ranks [1, r1, .., 1] */
  const int32_t* p_tables;      /* NULL: every table has the row factors p[] */
} ttx_geom;

const char* ttx_last_error(void);
int ttx_version(void);

/* ------------------------------------------------------------------ plan ---
 * The lookup plan is this library's replacement for the reference's per-chunk
 * pointer-array set-up kernels (init_batch_gemm_{forward,backward}_*T_kernel,
 * tt_embeddings_cuda.cu:79-360, :754-918): index decode, a stable radix sort of
 * the lookups by (table, i_t) for every core and the work-list of index groups
 * that share a middle-core slice.  It depends only on (geometry, indices,
 * tableidx, rowidx); forward and backward of the same batch can share one plan.
 * rowidx may be NULL (the backward kernel then gathers the bag row per lookup).
 * Passing plan == NULL to ttx_tt_forward / ttx_tt_backward builds it inside
 * their workspace.
 * With FOUR cores on the three-core kernels a plan also carries the product of each
 * lookup's last two core slices, left there by the latest ttx_tt_forward on that plan;
 * a ttx_tt_backward on the same plan, with cores 2 and 3 at the same addresses, reads it
 * instead of recomputing it.  This library's fused optimizers and ttx_plan_build drop it;
 * a caller who rewrites cores 2 / 3 by other means BETWEEN the forward and the backward
 * of one plan (nothing in the reference's flow does) must rebuild the plan first. */
size_t ttx_plan_bytes(const ttx_geom* g, int64_t nnz);
int ttx_plan_build(const ttx_geom* g, int64_t nnz, const int64_t* indices,
                   const int64_t* tableidx, const int64_t* rowidx, void* plan,
                   size_t plan_bytes, ttx_stream_t stream);

/* --------------------------------------------------------------- forward ---
 * replaces tt_embeddings_forward_cuda (tt_embeddings.cpp:13-26,
 * tt_embeddings_cuda.cu:964-1075).  output[num_tables,B,D] is overwritten with
 * the bag sums of the first `nnz` lookups (zeros when nnz == 0).  D may be any
 * positive value (the reference requires D % 4 == 0). */
size_t ttx_tt_forward_workspace_bytes(const ttx_geom* g, int32_t B, int32_t D,
                                      int64_t nnz);
int ttx_tt_forward(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz,
                   const int64_t* indices, const int64_t* rowidx,
                   const int64_t* tableidx, const float* const* tt_cores,
                   float* output, const void* plan, void* workspace,
                   size_t workspace_bytes, ttx_stream_t stream);

/* nn.EmbeddingBag's per_sample_weights (not in the reference): lookup n enters its
 * bag scaled by per_sample_weights[n], and its share of the bag gradient is scaled the same way in
 * ttx_tt_backward_w.  NULL = the plain entry point. */
int ttx_tt_forward_w(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz,
                     const int64_t* indices, const int64_t* rowidx, const int64_t* tableidx,
                     const float* per_sample_weights, const float* const* tt_cores,
                     float* output, const void* plan, void* workspace, size_t workspace_bytes,
                     ttx_stream_t stream);

/* ... and with a gradient for the weights: ttx_tt_forward_wr leaves the lookups' rows (unweighted, [nnz, D], 16-byte
 * aligned) in rows_keep (NULL = ttx_tt_forward_w), and ttx_psw_backward turns them into
 * d_psw[n] = <d_output[tableidx[n], rowidx[n], :], rows[n, :]>, what autograd gives nn.EmbeddingBag(mode="sum"). */
int ttx_tt_forward_wr(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz,
                      const int64_t* indices, const int64_t* rowidx, const int64_t* tableidx,
                      const float* per_sample_weights, const float* const* tt_cores,
                      float* output, float* rows_keep, const void* plan, void* workspace,
                      size_t workspace_bytes, ttx_stream_t stream);

/* Not in the reference (round 4): the cache-live forward of ONE table in one call -- tt_embeddings_forward_cuda on the misses
 * followed by cache_forward_cuda (tt_embeddings_cuda.cu:1498-1572) on the hits -- with the bag sums of both parts in ONE launch.
 * The batch is the partitioned one of ttx_preprocess_indices_async: `nnz` lookups, the misses in front; `plan` is the plan of the
 * misses (ttx_plan_build_n with the device-side split point), `rowidx` / `cache_loc` are the partitioned bag rows / cache
 * locations of all `nnz` positions.  A bag's row receives at most two terms (its contraction sum, its cache sum) through fp32
 * atomics on the zeroed output: the result does not depend on their order.  ttx_tt_forward_cached_supported says whether the
 * call is taken this way (one table, D % 4 == 0, at most 65536 lookups); otherwise run ttx_tt_forward + ttx_cache_forward_n. */
int ttx_tt_forward_cached_supported(const ttx_geom* g, int32_t D, int64_t nnz);
int ttx_tt_forward_cached(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz,
                          const int64_t* indices, const int64_t* rowidx, const int64_t* tableidx,
                          const float* const* tt_cores, const int32_t* cache_loc, const float* cache_weight,
                          float* output, const void* plan, void* workspace, size_t workspace_bytes,
                          ttx_stream_t stream);

/* Not in the reference: ttx_tt_forward_wr with the bag pooling done INSIDE the contraction kernel (no pooling launch:
 * the lookup that completes a bag sums its rows in index order, same result bit for bit) where the shape and the
 * batch allow it -- the call falls back to the separate pooling launch otherwise, so it is always valid.
 *   offsets  [num_tables * B + 1] int64: the bags' extents in the table-major, include_last_offset form the rowidx /
 *            tableidx arrays were derived from (tt_embeddings_ops.py:851; every lookup of bag b at [offsets[b], offsets[b+1]))
 *   arrive   device array of ttx_tt_forward_arrive_ints() int32, ALL ZERO on entry; all zero again when the call's
 *            kernels have run (keep one per stream, zero it once).  NULL / 0 ints: pooling stays a launch of its own. */
int64_t ttx_tt_forward_arrive_ints(const ttx_geom* g, int64_t nnz);
int ttx_tt_forward_o(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz, const int64_t* indices,
                     const int64_t* rowidx, const int64_t* tableidx, const float* per_sample_weights,
                     const float* const* tt_cores, float* output, float* rows_keep, const int64_t* offsets,
                     int32_t* arrive, const void* plan, void* workspace, size_t workspace_bytes, ttx_stream_t stream);
int ttx_psw_backward(int32_t B, int32_t D, int64_t nnz, const float* rows, const int64_t* rowidx,
                     const int64_t* tableidx, const float* d_output, float* d_psw, ttx_stream_t stream);

/* decompress rows: rows[n, :] = TT row of indices[n] in table tableidx[n]
 * (tableidx == NULL -> table 0).  This is the contraction alone, the part of
 * prefetch_cached_weights_cuda (tt_embeddings_cuda.cu:1156-1258) that fills
 * cache_weight.  Same workspace size as ttx_tt_forward with B = 0. */
int ttx_tt_rows(const ttx_geom* g, int32_t D, int64_t nnz,
                const int64_t* indices, const int64_t* tableidx,
                const float* const* tt_cores, float* rows, void* workspace,
                size_t workspace_bytes, ttx_stream_t stream);

/* -------------------------------------------------------------- backward ---
 * replaces tt_embeddings_backward_{dense,sgd,adagrad}_cuda
 * (tt_embeddings.cpp:28-72, tt_embeddings_cuda.cu:419-752).
 *  optim == TTX_OPTIM_DENSE  : d_tt_cores[t] (full core shape) is overwritten
 *                              with the gradient; cores untouched.
 *  optim == TTX_OPTIM_SGD    : cores  -= lr * g              (every element)
 *  optim == TTX_OPTIM_ADAGRAD: state += g*g;
 *                              cores  -= lr * g / (sqrtf(state) + eps)
 * Gradients of duplicate lookups are summed before the single optimizer step.
 * Unlike the reference's apply kernels (tt_embeddings_cuda.cu:612-648, whose
 * grid covers only part of each core when p[t] > r*q*r) every touched slice is
 * updated; slices with no lookup have g == 0 and are left unchanged. */
size_t ttx_tt_backward_workspace_bytes(const ttx_geom* g, int32_t B, int32_t D,
                                       int64_t nnz);
int ttx_tt_backward(const ttx_geom* g, int32_t optim, int32_t B, int32_t D,
                    float learning_rate, float eps, int64_t nnz,
                    const int64_t* indices, const int64_t* rowidx,
                    const int64_t* tableidx, const float* d_output,
                    float* const* tt_cores, float* const* optimizer_state,
                    float* const* d_tt_cores, const void* plan, void* workspace,
                    size_t workspace_bytes, ttx_stream_t stream);

int ttx_tt_backward_w(const ttx_geom* g, int32_t optim, int32_t B, int32_t D,
                      float learning_rate, float eps, int64_t nnz, const int64_t* indices,
                      const int64_t* rowidx, const int64_t* tableidx,
                      const float* per_sample_weights, const float* d_output,
                      float* const* tt_cores, float* const* optimizer_state,
                      float* const* d_tt_cores, const void* plan, void* workspace,
                      size_t workspace_bytes, ttx_stream_t stream);

/* Not in the reference (round 4): ttx_tt_backward_w of a cache-live batch with the cache rows' scatter
 * (cache_backward_sgd_cuda / _dense, tt_embeddings_cuda.cu:1574-1697: cache_dst[loc[n], :] += cache_scale * cache_grad[rowidx[n], :]
 * for the lookups behind the device-side split point *skip_dev) done by work-groups of the optimizer's launch instead of a launch of
 * its own.  *tail_done = 1 when it was; 0 (four-core route, an empty batch, switched off) = the caller runs
 * ttx_cache_backward_sgd_n / _dense_n itself.  rowidx is the partitioned bag rows of all nnz positions, as for ttx_tt_forward_cached. */
int ttx_tt_backward_wc(const ttx_geom* g, int32_t optim, int32_t B, int32_t D, float lr, float eps,
                       int64_t nnz, const int64_t* indices, const int64_t* rowidx,
                       const int64_t* tableidx, const float* per_sample_weights, const float* d_output,
                       float* const* tt_cores, float* const* optimizer_state, float* const* d_tt_cores,
                       const void* plan, void* workspace, size_t workspace_bytes, ttx_stream_t stream,
                       const int32_t* skip_dev, const int32_t* cache_loc, const float* cache_grad, float cache_scale,
                       float* cache_dst, int32_t* tail_done);

/* ------------------------------ pooling modes: mean and max (not in the reference) -----
 * nn.EmbeddingBag(mode="mean" / "max") over the same contraction (the reference pools by sum only).  Bags are described
 * by offsets [nb + 1] int64 (closing entry included, table-major over the tables as everywhere): bag b covers positions
 * [offsets[b], offsets[b + 1]) of the batch.  No atomics, one writer per element: bit-identical from run to run, nothing
 * read back (capturable).  Float arrays 16-byte aligned with D % 4 == 0 take the float4 kernels, anything else the scalar ones.
 *
 *   ttx_bag_mean_scale         y[b, :] = x[b, :] / max(1, offsets[b + 1] - offsets[b]), x / y [nb, D] (y may be x): the mean
 *                              from the bag sum of ttx_tt_forward*, and the share of a bag's gradient each lookup receives
 *                              (scale d_output, then any sum-mode backward).  An empty bag stays 0.
 *   ttx_tt_rows_p              ttx_tt_rows with a prebuilt plan (NULL = ttx_tt_rows): rows [nnz, D] (16-byte aligned) of a
 *                              plan from ttx_plan_build with rowidx == NULL.  No workspace when a plan is given.  A four-core
 *                              plan keeps the merged last cores of the call for ttx_tt_backward_rows on the same plan.
 *   ttx_bag_max_pool           output [nb, D] = column-wise max over the bag's rows [nnz, D], argmax [nb, D] int32 = the
 *                              position n (row of `rows`) that holds it: the lowest one on a tie (PyTorch's order: a strict >
 *                              scanning the bag in index order).  Empty bag: 0 and -1.  One wave per bag.
 *   ttx_bag_max_pool_backward  d_rows [nnz, D] = argmax[bag(n), e] == n ? d_output[bag(n), e] : 0 -- every element written
 *                              once (lookups outside every bag: 0); no memset needed in front.
 *   ttx_tt_backward_rows       ttx_tt_backward with ONE gradient row PER LOOKUP: lookup n's gradient is d_rows[n, :]
 *                              ([nnz, D]) instead of d_output[tableidx[n], rowidx[n], :].  Same optimizers, same outputs.
 *                              plan: NULL (built in the workspace), or the plan of ttx_tt_rows_p -- built WITHOUT bag rows
 *                              (ttx_plan_build rowidx == NULL; a plan that carries bag rows addresses the wrong rows).
 *                              Workspace: ttx_tt_backward_rows_workspace_bytes (the backward's plus nnz int64). */
int ttx_bag_mean_scale(int64_t nb, int32_t D, const int64_t* offsets, const float* x, float* y, ttx_stream_t stream);
int ttx_tt_rows_p(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                  const float* const* tt_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                  ttx_stream_t stream);
int ttx_bag_max_pool(int64_t nb, int32_t D, int64_t nnz, const int64_t* offsets, const float* rows, float* output,
                     int32_t* argmax, ttx_stream_t stream);
int ttx_bag_max_pool_backward(int64_t nb, int32_t D, int64_t nnz, const int64_t* offsets, const int32_t* argmax,
                              const float* d_output, float* d_rows, ttx_stream_t stream);
size_t ttx_tt_backward_rows_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz);
int ttx_tt_backward_rows(const ttx_geom* g, int32_t optim, int32_t D, float learning_rate, float eps, int64_t nnz,
                         const int64_t* indices, const int64_t* tableidx, const float* d_rows,
                         float* const* tt_cores, float* const* optimizer_state, float* const* d_tt_cores,
                         const void* plan, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ------------------------------ padded bags: padding_idx (not in the reference) -----
 * nn.EmbeddingBag(padding_idx=) and its 2-D fixed-length input: a ragged batch fed with static shapes, every bag padded to
 * L slots with one index value.  ttx_bags_compact turns the padded bags into ragged bags plus a device-side live count --
 * what ttx_lookup_prologue_n takes -- so the padding costs no contraction, is not counted in the frequency table and
 * the step stays capturable.  A stable stream compaction by flag (indices[i] != padding_idx):
 *
 *   out_indices[0 .. n)    the live slots IN THEIR ORIGINAL ORDER (the order inside a bag decides a tie of the max mode and
 *                          the order of the fp32 bag sum); out_indices[n .. nnz) = 0.  Every element has exactly one writer,
 *                          no memset runs in front: the buffer is a function of the input alone.
 *   out_offsets[b]         live slots in front of bag b, b < nb; out_offsets[nb] = *n_live = n.  Empty bags and bags of
 *                          padding only give equal consecutive entries.
 *   bags                   offsets != NULL: nb + 1 int64 entries, closing one included, offsets[0] = 0 and offsets[nb] = nnz as
 *                          everywhere (entries are clamped to [0, nnz]); offsets == NULL: bag b is slots [b L, (b + 1) L) and
 *                          nnz == nb L.
 *   nnz == 0 or nb == 0    returns 0 after zeroing out_offsets (nb + 1 entries) and *n_live where those pointers are not NULL.
 *   errors                 negative sizes, nnz >= 2^31, NULL indices / outputs / workspace, offsets == NULL with nnz != nb L,
 *                          a workspace below ttx_bags_compact_workspace_bytes or not 8-byte aligned: -1 with ttx_last_error()
 *                          set, before anything touches a device.
 *   launches               one up to 32768 slots (every work-group builds the rank table of the whole batch in LDS itself);
 *                          above that a count and a scatter launch over tiles of >= 4096 slots (at most 1024 tiles) and,
 *                          with offsets given as an array, a third that gathers the bag starts.
 *                          No atomics, no work-group waits on another inside a launch: bit-identical from run to run, nothing
 *                          read back (capturable).  indices 16-byte aligned: two slots per 16-byte load. */
size_t ttx_bags_compact_workspace_bytes(int64_t nb, int64_t nnz);
int ttx_bags_compact(int64_t nb, int64_t nnz, const int64_t* indices, const int64_t* offsets, int64_t L, int64_t padding_idx,
                     int64_t* out_indices, int64_t* out_offsets, int32_t* n_live, void* workspace, size_t workspace_bytes,
                     ttx_stream_t stream);

/* ------------------------------ unpooled rows at padded positions (not in the reference) -----
 * nn.Embedding(padding_idx=): one row per position, the padding positions zero.  The positions are compacted as n bags of ONE
 * slot (ttx_bags_compact, offsets == NULL, L = 1), the live ones are planned with the device-side count (ttx_plan_build_n),
 * contracted (ttx_tt_rows_p) and trained (ttx_tt_backward_rows); these two calls carry rows between the compacted order and
 * the positions:
 *
 *   rank [n + 1]           ttx_bags_compact's out_offsets of that call: rank[i] = live positions in front of i.  Position i is
 *                          live iff rank[i + 1] > rank[i]; rank[i] is clamped to [0, n - 1] before it addresses anything.
 *   ttx_rows_expand        out[i, :] = live(i) ? rows[rank[i], :] : 0 for i < n; rows / out [n, D].  Every element of `out` has
 *                          exactly one writer, no memset runs in front; rows of padding positions are not read.
 *   ttx_rows_collect       d_rows[rank[i], :] = d_out[i, :] for the live i only; d_out / d_rows [n, D].  Rows of d_rows at and
 *                          beyond rank[n] are not written (and, a plan's kernels being driven by its live count, not read).
 *   n == 0                 returns 0 and launches nothing.
 *   errors                 n < 0, D <= 0, n >= 2^31, a NULL pointer with n > 0, a float pointer not 4-byte aligned (rank not
 *                          8-byte aligned): -1 with ttx_last_error() set, before anything touches a device.
 *   kernels                D % 4 == 0 and the float pointers 16-byte aligned: 16-byte loads and stores (rows_expand4_kernel /
 *                          rows_collect4_kernel), anything else float by float (rows_expand1_kernel / rows_collect1_kernel).
 *                          Consecutive lanes hold consecutive pieces of the position-ordered array, short rows are grouped into
 *                          one work-group's tile; element offsets are 64-bit.  No atomics, no LDS, no workspace, nothing read
 *                          back: bit-identical from run to run, capturable. */
int ttx_rows_expand(int64_t n, int32_t D, const int64_t* rank, const float* rows, float* out, ttx_stream_t stream);
int ttx_rows_collect(int64_t n, int32_t D, const int64_t* rank, const float* d_out, float* d_rows, ttx_stream_t stream);

/* ------------------------------ unpooled rows with a live cache (not in the reference) -----
 * nn.Embedding on a table whose row cache is live: the N positions (padding dropped first: ttx_bags_compact over one-slot bags)
 * go through the live preprocess (ttx_preprocess_indices_async with offsets = N one-slot bags, or = rank with padding), which
 * leaves the n live lookups in PARTITION order -- the misses, in their order, in [0, n_tt), the hits in [n_tt, n) -- with the
 * split point on the device.  The misses are planned (ttx_plan_build_n), contracted (ttx_tt_rows_p) and trained
 * (ttx_tt_backward_rows); the hits' rows are trained in place (ttx_cache_backward_*_n / ttx_cache_backward_sorted with
 * rowidx = pos, skip_dev = n_tt_dev, on the gradient [N, D] itself).  These two calls carry rows between partition order and the
 * positions:
 *
 *   pos [n]                part_rowidx of that preprocess: the position of partition slot s; clamped to [0, N - 1] before it
 *                          addresses anything.  Injective onto the live positions.
 *   loc [n]                part_cache_locations: slot s's cache row for s >= n_tt (-1 in front of it, where it is not read);
 *                          clamped to [0, cache_size - 1] before it addresses anything.
 *   n_tt, n_tt_dev         the split point: *n_tt_dev (a device int32, clamped to [0, n]) -- or, n_tt_dev == NULL, the host's n_tt:
 *                          NULL gives the plain entry point.  n_tt <= n is checked either way (pass n with a device count).
 *   rank                   NULL: no padding, n == N.  Else ttx_bags_compact's out_offsets [N + 1] as for ttx_rows_expand:
 *                          position i is padding iff not rank[i + 1] > rank[i].
 *   ttx_rows_place         out[pos[s], :] = s < n_tt ? rows_tt[s, :] : cache_weight[loc[s], :] for s < n, and out[i, :] = 0 for
 *                          every padding position i < N; rows_tt [>= n_tt, D] (read for s < n_tt only), cache_weight
 *                          [cache_size, D], out [N, D].  The gather of the cache rows is part of the launch: there is no rows
 *                          buffer for the hits.  Every element of `out` has exactly one writer, no memset runs in front.
 *   ttx_rows_pick          d_rows[s, :] = d_out[pos[s], :] for s < n_tt only; d_out [N, D], d_rows [>= n_tt, D].  Rows of d_rows at
 *                          and beyond n_tt are not written (and, a plan's kernels being driven by its count, not read).
 *   N == 0 or n == 0       returns 0; with N > 0, n == 0 and a rank ttx_rows_place still zeroes the (padding) rows.
 *   errors                 a negative size, D <= 0, N >= 2^31, n > N, n_tt > n, rank == NULL with n != N, cache_size <= 0 while
 *                          n_tt < n with a host count, a NULL pointer that would be dereferenced (with a device count: any of them),
 *                          a float / int32 pointer not 4-byte aligned, pos / rank not 8-byte aligned: -1 with ttx_last_error()
 *                          set, before anything touches a device.
 *   kernels                D % 4 == 0 and the float pointers 16-byte aligned: 16-byte loads and stores (rc_place4_kernel /
 *                          rc_pick4_kernel), anything else float by float (rc_place1_kernel / rc_pick1_kernel).  Consecutive lanes
 *                          hold consecutive pieces of a row, short rows are grouped into one work-group's tile, the grid is capped
 *                          and strides over the tiles; element offsets are 64-bit.  One launch each.  No atomics, no LDS, no
 *                          workspace, nothing read back: bit-identical from run to run, capturable. */
int ttx_rows_place(int64_t N, int64_t n, int64_t n_tt, const int32_t* n_tt_dev, int32_t D, const int64_t* pos, const int32_t* loc,
                   const float* rows_tt, const float* cache_weight, int64_t cache_size, const int64_t* rank, float* out,
                   ttx_stream_t stream);
int ttx_rows_pick(int64_t N, int64_t n, int64_t n_tt, const int32_t* n_tt_dev, int32_t D, const int64_t* pos, const float* d_out,
                  float* d_rows, ttx_stream_t stream);

/* ------------------------------ merged bags: per-table batches -> one table-major batch (not in the reference) -----
 * Tables of different cardinality arrive as one (indices, bags[, weights]) batch per table (DLRM's call form); the table-batched
 * lookup takes ONE batch, table-major.  ttx_bags_merge builds it in one launch per TTX_MAX_TABLES_MIXED tables -- concatenate,
 * shift the bag starts, widen int32, fill in default weights, mark the padding -- with nothing read back and no pointer table
 * copied to the device: every per-table argument below is a HOST array of ntab entries that travels by value in the kernel's
 * argument block (64 tables take 2.6 KiB of the 4 KiB segment).
 *
 *   indices[k], nnz[k]     table k's slots: a device pointer (may be NULL when nnz[k] == 0) to int64, or int32 where
 *                          index_bytes[k] == 4 (index_bytes == NULL: all int64), aligned to its element.
 *   offsets[k]             table k's B bag starts (device pointer, int64, or int32 where offset_bytes[k] == 4; entries behind the
 *                          first B -- the closing one of the include_last_offset form -- are not read), or NULL: B bags of L[k]
 *                          slots each, nnz[k] == B * L[k] (the 2-D form; L[k] is ignored where offsets[k] is given).
 *   weights                NULL: no table has weights and out_weights is not written.  Else weights[k] = table k's nnz[k] floats
 *                          or NULL for 1.0f.
 *   padding, has_padding   padding == NULL: none.  Else a slot of table k that equals padding[k] is written as `sentinel` where
 *                          has_padding[k] != 0; every other slot is copied.
 *   out_indices [N]        int64, N = sum nnz[k]: table k's slots at base_k = sum_{j<k} nnz[j], in order.
 *   out_offsets [ntab B+1] int64: entry k B + b = base_k + min(max(start_k[b], 0), nnz[k]); the last entry = N.
 *   out_weights [N]        float.
 *   N == 0 or B == 0       the offsets owed are still written (at least the closing entry).
 *   errors                 ntab < 1, N >= 2^31, a negative size, NULL where a pointer is owed, a pointer not aligned to its
 *                          element, an element width other than 4 / 8, nnz[k] != B L[k] without offsets: -1 with
 *                          ttx_last_error() set, before anything touches a device.
 * Every output element has exactly one writer; no atomics, no memset, no workspace, no work-group waits on another: the
 * buffers are a function of the inputs alone, bit-identical from run to run, and the call is capturable.  For int64 inputs
 * without padding the result is, integer for integer, the concatenation torch would build. */
int ttx_bags_merge(int32_t ntab, int64_t B, int32_t include_last_offset, const void* const* indices, const int64_t* nnz,
                   const int32_t* index_bytes, const void* const* offsets, const int32_t* offset_bytes, const int64_t* L,
                   const float* const* weights, const int64_t* padding, const uint8_t* has_padding, int64_t sentinel,
                   int64_t* out_indices, int64_t* out_offsets, float* out_weights, ttx_stream_t stream);

/* ----------------------------------------------- duplicate lookups -----
 * Not in the reference (which contracts every lookup on its own): a batch's lookups are mapped onto their
 * DISTINCT (table, index) pairs, the contraction runs once per pair, bag pooling gathers each lookup's row
 * through the map (same sums in the same order: the output is bit-identical to ttx_tt_forward's), and the
 * backward first adds up, in a fixed order, the bag gradients of a pair's occurrences -- one contraction, one
 * set of partial gradients per pair.  Pays on large batches that repeat rows (Zipf 1.2, 327k lookups: 0.79 ->
 * 0.35 ms/step); on a uniform stream it only adds the key sort and the launches of the map.
 *
 *   ttx_dedup_bytes     size of the map buffer; 0 = this batch is not deduplicated (per-table row factors, a
 *                       key space num_tables * prod(p) beyond 2^61, nnz >= 2^31): use the plain entry points.
 *   ttx_dedup_build     builds the map (<= 16384 lookups with 32-bit keys: one work-group sorts the keys in LDS;
 *                       otherwise a multi-work-group stable radix sort of 64-bit keys -- deterministic either
 *                       way, nothing read back: capturable) AND the lookup plan of the distinct pairs into
 *                       `plan` (ttx_plan_bytes(g, nnz) bytes).
 *   ttx_tt_forward_dd / ttx_tt_backward_dd   as ttx_tt_forward_w / ttx_tt_backward_w (psw may be NULL), driven
 *                       by a map + plan built for the same (indices, tableidx). */
size_t ttx_dedup_bytes(const ttx_geom* g, int64_t nnz);
int ttx_dedup_build(const ttx_geom* g, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                    void* dedup, size_t dedup_bytes, void* plan, size_t plan_bytes, ttx_stream_t stream);
size_t ttx_tt_forward_dd_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz);
int ttx_tt_forward_dd(const ttx_geom* g, int32_t B, int32_t D, int64_t nnz, const int64_t* rowidx,
                      const int64_t* tableidx, const float* per_sample_weights, const void* dedup,
                      const void* plan, const float* const* tt_cores, float* output, void* workspace,
                      size_t workspace_bytes, ttx_stream_t stream);
size_t ttx_tt_backward_dd_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz);
int ttx_tt_backward_dd(const ttx_geom* g, int32_t optim, int32_t B, int32_t D, float learning_rate, float eps,
                       int64_t nnz, const int64_t* rowidx, const int64_t* tableidx,
                       const float* per_sample_weights, const float* d_output, const void* dedup,
                       const void* plan, float* const* tt_cores, float* const* optimizer_state,
                       float* const* d_tt_cores, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ------------------------------------------- core-0 row split (not in the reference) -----
 * A T = 3 table whose first factor is q0 = k q0' (q0 = 8: k = 2, q0' = 4) is contracted as k PART lookups per index
 * in the table p' = [k p0, p1, p2], q' = [q0', q1, q2]: core 0 [p0, q0, r1] is, element for element, [k p0, q0', r1]; index
 * (i0, i1, i2) becomes (k i0 + h, i1, i2), h = 0..k-1, and part h of bag b is bag k b + h of a batch with k nb bags and
 * D / k columns -- an output [nb, D] row-major IS [k nb, D / k], so nothing is copied back.  This is how factorings with
 * q0 > 4 (the reference's default for D = 512, [8,8,8]) reach the shape-specialised kernels (q0 <= 4): same sums, the
 * core-1 / core-2 gradients of the parts add up in the ordinary reduction.  `offsets` holds nb + 1 entries (closing entry
 * included), bags table-major as everywhere; out_indices [k nnz], out_offsets [k nb + 1].  p_rest = p1 * p2. */
int ttx_split0_expand(int64_t nnz, int64_t nb, int32_t k, int64_t p_rest, const int64_t* indices, const int64_t* offsets,
                      int64_t* out_indices, int64_t* out_offsets, ttx_stream_t stream);

/* ------------------------------------------------------ software cache -----
 * replaces update_cache_state_cuda (tt_embeddings.cpp:74,
 * tt_embeddings_cuda.cu:1077-1113): cache_freq[slot(idx)] += 1 with at most 3
 * linear probes of an open-addressing table keyed by a murmur3-style hash
 * (hashtbl_cuda_utils.cuh:48-76, :102-133). */
int ttx_update_cache_state(int64_t nnz, const int64_t* indices,
                           int64_t hashtbl_size, int64_t* hashtbl,
                           int64_t* cache_freq, ttx_stream_t stream);

/* replaces preprocess_indices_sync_cuda (tt_embeddings.cpp:88-95,
 * tt_embeddings_cuda.cu:1377-1496).
 *  rowidx/tableidx[nnz] are always written (bag b covers
 *  [offsets[b], offsets[b+1]); rowidx = b % B, tableidx = b / B).
 *  If warmup != 0 or num_tables != 1 nothing else happens, *num_tt_host = nnz
 *  and *partitioned_host = 0.  Otherwise every index is looked up in the
 *  hash table; lookups whose slot has a cache row go to the REAR of
 *  part_colidx / part_rowidx / part_cache_locations in reverse order, the rest
 *  keep their order at the front (cub::DevicePartition::Flagged semantics), the
 *  count of front entries is copied to *num_tt_host after a stream
 *  synchronise, and *partitioned_host = 1.  part_cache_locations of front
 *  entries is -1 (uninitialised in the reference). */
size_t ttx_preprocess_workspace_bytes(int64_t nnz);
int ttx_preprocess_indices_sync(int64_t nnz, const int64_t* colidx,
                                int64_t num_bags_total, const int64_t* offsets,
                                int32_t num_tables, int32_t warmup,
                                int64_t hashtbl_size, const int64_t* hashtbl,
                                const int32_t* cache_state, int64_t* rowidx,
                                int64_t* tableidx, int64_t* part_colidx,
                                int64_t* part_rowidx,
                                int32_t* part_cache_locations,
                                int32_t* num_tt_host, int32_t* partitioned_host,
                                void* workspace, size_t workspace_bytes,
                                ttx_stream_t stream);

/* The same, with update_cache_state folded into the first kernel when upd_hashtbl /
 * upd_cache_freq are non-NULL (one launch instead of two; the order "count the batch's
 * indices, then look them up" of tt_embeddings_ops.py:827-846 is kept). */
int ttx_preprocess_indices_sync_fused(int64_t nnz, const int64_t* colidx,
                                      int64_t num_bags_total, const int64_t* offsets,
                                      int32_t num_tables, int32_t warmup,
                                      int64_t hashtbl_size, const int64_t* hashtbl,
                                      const int32_t* cache_state, int64_t* rowidx,
                                      int64_t* tableidx, int64_t* part_colidx,
                                      int64_t* part_rowidx, int32_t* part_cache_locations,
                                      int32_t* num_tt_host, int32_t* partitioned_host,
                                      int64_t* upd_hashtbl, int64_t* upd_cache_freq,
                                      void* workspace, size_t workspace_bytes,
                                      ttx_stream_t stream);

/* ---- device-side counts: the cache-live path without its host read-back -------------------
 * The reference copies the partition's split point to the host and synchronises
 * (tt_embeddings_cuda.cu:1481-1488) because its launch grids depend on it.  Here every kernel
 * can take its lookup count from device memory instead, with the host-side `nnz` an upper bound
 * that only sizes grids and workspaces:
 *  - ttx_preprocess_indices_async: as ttx_preprocess_indices_sync_fused, but when num_tt_dev
 *    (a device int32) is non-NULL the count of TT entries is written there and nothing is read
 *    back (*num_tt_host keeps nnz);
 *  - ttx_plan_build_n: nnz_dev (device int32, <= nnz) is the number of leading entries of
 *    indices / tableidx / rowidx to plan; a plan built this way may be handed to
 *    ttx_tt_forward / ttx_tt_backward together with the same upper bound nnz (their kernels
 *    are driven by the plan; workspaces are sized for nnz);
 *  - ttx_cache_*_n: skip_dev (device int32) = number of leading entries of cache_locations /
 *    rowidx that are NOT cached; the kernels work on [*skip_dev, nnz).
 * Passing NULL for the device pointer gives exactly the plain entry point. */
int ttx_preprocess_indices_async(int64_t nnz, const int64_t* colidx, int64_t num_bags_total,
                                 const int64_t* offsets, int32_t num_tables, int32_t warmup,
                                 int64_t hashtbl_size, const int64_t* hashtbl,
                                 const int32_t* cache_state, int64_t* rowidx, int64_t* tableidx,
                                 int64_t* part_colidx, int64_t* part_rowidx,
                                 int32_t* part_cache_locations, int32_t* num_tt_host,
                                 int32_t* partitioned_host, int32_t* num_tt_dev,
                                 int64_t* upd_hashtbl, int64_t* upd_cache_freq, void* workspace,
                                 size_t workspace_bytes, ttx_stream_t stream);
int ttx_plan_build_n(const ttx_geom* g, int64_t nnz, const int32_t* nnz_dev, const int64_t* indices,
                     const int64_t* tableidx, const int64_t* rowidx, void* plan, size_t plan_bytes,
                     ttx_stream_t stream);
int ttx_cache_forward_n(int32_t B, int64_t nnz, const int32_t* skip_dev, const int32_t* cache_locations,
                        const int64_t* rowidx, int32_t D, const float* cache_weight, float* output,
                        ttx_stream_t stream);
int ttx_cache_backward_sgd_n(int64_t nnz, const int32_t* skip_dev, int32_t D, const float* grad_output,
                             const int32_t* cache_locations, const int64_t* rowidx, float learning_rate,
                             float* cache_weight, ttx_stream_t stream);
int ttx_cache_backward_dense_n(int64_t nnz, const int32_t* skip_dev, int32_t D, const float* grad_output,
                               const int32_t* cache_locations, const int64_t* rowidx, int64_t cache_size,
                               float* grad_cache_weight, ttx_stream_t stream);
int ttx_cache_backward_rowwise_adagrad_approx_n(int64_t nnz, const int32_t* skip_dev, int32_t D,
                                                const float* grad_output, const int32_t* cache_locations,
                                                const int64_t* rowidx, float learning_rate, float eps,
                                                float* cache_optimizer_state, float* cache_weight,
                                                ttx_stream_t stream);

/* nn.EmbeddingBag's per_sample_weights with a LIVE cache (not in the reference, which has no weights at all):
 *  - ttx_preprocess_indices_async_w: as ttx_preprocess_indices_async; the weights travel with their lookups into
 *    partitioned_weights and every partitioned entry's original position goes to partitioned_origin (either may be
 *    NULL), so that the gradient of the weights can be handed back in the caller's order;
 *  - ttx_cache_forward_nw: output[rowidx[n]] += per_sample_weights[n] * cache_weight[loc[n]] for the cached entries
 *    (per_sample_weights == NULL: ttx_cache_forward_n);
 *  - ttx_cache_rows_n: rows[n] = cache_weight[loc[n]] for the cached entries -- with the contraction's rows of the
 *    misses in front (ttx_tt_forward_wr) ttx_psw_backward then yields d per_sample_weights for the whole batch;
 *  - ttx_cache_weighted_grad_n: scaled[n] = per_sample_weights[n] * grad_output[rowidx[n]] for the cached entries
 *    (n >= *skip_dev), scaled[n] = 0 in front of them (where neither rowidx nor the weight is read) and iota[n] = n for
 *    EVERY n -- both outputs are written whole: ttx_cache_backward_*_n / ttx_cache_backward_sorted(.., grad_output =
 *    scaled, rowidx = iota, num_bags = nnz, ..) is the weighted backward. */
int ttx_preprocess_indices_async_w(int64_t nnz, const int64_t* colidx, int64_t num_bags_total, const int64_t* offsets,
                                   int32_t num_tables, int32_t warmup, int64_t hashtbl_size, const int64_t* hashtbl,
                                   const int32_t* cache_state, int64_t* rowidx, int64_t* tableidx,
                                   int64_t* partitioned_colidx, int64_t* partitioned_rowidx, int32_t* cache_locations,
                                   int32_t* num_tt_host, int32_t* partitioned_host, int32_t* num_tt_dev,
                                   int64_t* upd_hashtbl, int64_t* upd_cache_freq, const float* per_sample_weights,
                                   float* partitioned_weights, int32_t* partitioned_origin, void* workspace,
                                   size_t workspace_bytes, ttx_stream_t stream);
int ttx_cache_forward_nw(int32_t B, int64_t nnz, const int32_t* skip_dev, const int32_t* cache_locations,
                         const int64_t* rowidx, const float* per_sample_weights, int32_t D, const float* cache_weight,
                         float* output, ttx_stream_t stream);
int ttx_cache_rows_n(int64_t nnz, const int32_t* skip_dev, const int32_t* cache_locations, int32_t D,
                     const float* cache_weight, float* rows, ttx_stream_t stream);
int ttx_cache_weighted_grad_n(int64_t nnz, const int32_t* skip_dev, int32_t D, const float* grad_output,
                              const int64_t* rowidx, const float* per_sample_weights, float* scaled, int64_t* iota,
                              ttx_stream_t stream);

/* Lookup prologue of a batch while the cache is not live (warmup): what the module does
 * before the contraction -- update_cache_state (tt_embeddings_ops.py:827-833) when
 * upd_hashtbl / upd_cache_freq are non-NULL, preprocess_indices_sync with warmup = true
 * (:834-846: rowidx / tableidx from the offsets) and ttx_plan_build -- as ONE launch when the
 * batch qualifies (one table, every tables*p_t <= 256, 1024 < nnz <= 16384, <= 4096 bags),
 * otherwise as the separate launches; results are identical either way. */
int ttx_lookup_prologue(const ttx_geom* g, int64_t nnz, const int64_t* colidx,
                        int64_t num_bags_total, const int64_t* offsets, int64_t hashtbl_size,
                        int64_t* upd_hashtbl, int64_t* upd_cache_freq, int64_t* rowidx,
                        int64_t* tableidx, void* plan, size_t plan_bytes, ttx_stream_t stream);
/* The same with the number of LIVE lookups on the device (round 5; not in the reference): colidx holds nnz entries, the first
 * *nnz_dev of them (offsets[nb] == *nnz_dev <= nnz) are the batch -- only they are planned, and every call that later takes this
 * plan (ttx_tt_forward*, ttx_tt_backward*) works on exactly those, whatever nnz its launches are sized by.  nnz_dev == NULL: all
 * nnz.  For a table-sharded owner of RAGGED bags: fixed-capacity exchange buffers, no host read-back of the count.
 * (With a frequency table -- H > 0 -- only on the one-launch route; otherwise TTX_EUNSUPPORTED.) */
int ttx_lookup_prologue_n(const ttx_geom* g, int64_t nnz, const int64_t* colidx, int64_t nb, const int64_t* offsets,
                          int64_t H, int64_t* upd_hashtbl, int64_t* upd_cache_freq, int64_t* rowidx,
                          int64_t* tableidx, void* plan, size_t plan_bytes, const int32_t* nnz_dev, ttx_stream_t stream);

/* The prologues of SEVERAL batches in one launch (plan a round of training batches ahead: a batch's prologue depends on
 * its indices only, not on the cores).  colidx_host / offsets_host: HOST arrays of nbatch device pointers, every batch
 * with nnz indices and nb + 1 offsets; rowidx / tableidx: [nbatch][nnz]; plans: nbatch plan buffers plan_stride bytes
 * apart (a multiple of 256, >= ttx_plan_bytes(g, nnz)).  Batch z's results are exactly ttx_lookup_prologue's for that
 * batch; the frequency table counts all batches (counts commute).  One launch per 16 batches when the batch qualifies
 * for the single-launch prologue, the per-batch calls otherwise. */
int ttx_lookup_prologue_multi(const ttx_geom* g, int32_t nbatch, int64_t nnz, const int64_t* const* colidx_host,
                              int64_t num_bags_total, const int64_t* const* offsets_host, int64_t hashtbl_size,
                              int64_t* upd_hashtbl, int64_t* upd_cache_freq, int64_t* rowidx, int64_t* tableidx,
                              void* plans, size_t plan_stride, ttx_stream_t stream);

/* The same for a LIVE cache (one table; tt_embeddings_ops.py:827-846 with self.warmup == False, then the plan of the
 * misses): per batch z exactly ttx_preprocess_indices_async(num_tables = 1, warmup = 0, frequency update on the same
 * table, split point to num_tt_dev[z]) followed by ttx_plan_build_n(.., num_tt_dev + z, pcol_z, tableidx_z, prow_z) --
 * as three launches per 16 batches when the batch qualifies for the single-launch plan (every p_t <= 256, nnz <= 16384),
 * batch after batch otherwise.  rowidx / tableidx / pcol / prow / ploc: [nbatch][nnz]; num_tt_dev: [nbatch].  A cached
 * lookup's location depends on (hashtbl, cache_state) as the last ttx_cache_populate left them, not on the frequency
 * counts, so batch z's results do not depend on which other batches were counted first; they are void once the cache
 * is populated again. */
size_t ttx_lookup_prologue_cached_multi_workspace_bytes(int32_t nbatch, int64_t nnz);
int ttx_lookup_prologue_cached_multi(const ttx_geom* g, int32_t nbatch, int64_t nnz, const int64_t* const* colidx_host,
                                     int64_t num_bags, const int64_t* const* offsets_host, int64_t hashtbl_size,
                                     int64_t* hashtbl, int64_t* cache_freq, const int32_t* cache_state,
                                     int64_t* rowidx, int64_t* tableidx, int64_t* partitioned_colidx,
                                     int64_t* partitioned_rowidx, int32_t* cache_locations, int32_t* num_tt_dev,
                                     void* plans, size_t plan_stride, void* workspace, size_t workspace_bytes,
                                     ttx_stream_t stream);

/* replaces cache_populate_cuda (tt_embeddings.cpp:76-86,
 * tt_embeddings_cuda.cu:1260-1336): stable descending radix sort of the slots
 * by frequency, the top cache_size keys get cache rows (cache_state[slot] =
 * rank), the others are evicted from the table, and the cache rows are
 * decompressed from the TT cores. */
size_t ttx_cache_populate_workspace_bytes(const ttx_geom* g, int64_t hashtbl_size,
                                          int64_t cache_size, int32_t D);
int ttx_cache_populate(const ttx_geom* g, const float* const* tt_cores,
                       int64_t hashtbl_size, int64_t* hashtbl,
                       int64_t* cache_freq, int32_t* cache_state,
                       int64_t cache_size, int32_t D, float* cache_weight,
                       void* workspace, size_t workspace_bytes,
                       ttx_stream_t stream);
/* The same with per-call behaviour flags (round 6: the process-wide ttx_set_reference_exact of rounds 3-5 is gone).
 * TTX_POPULATE_REFERENCE_EXACT: cache_state[slot] of an EVICTED slot is left untouched, exactly as the reference's
 * mark_popular_colidx_kernel does (tt_embeddings_cuda.cu:1131-1133).  Default (flags = 0 = ttx_cache_populate): the slot's
 * cache row is dropped (cache_state = -1) -- otherwise, after a second populate, the next key inserted into that slot is
 * served, and trains, another index's cached row.  Identical on a first populate. */
#define TTX_POPULATE_REFERENCE_EXACT 1
int ttx_cache_populate_f(const ttx_geom* g, const float* const* tt_cores,
                         int64_t hashtbl_size, int64_t* hashtbl,
                         int64_t* cache_freq, int32_t* cache_state,
                         int64_t cache_size, int32_t D, float* cache_weight, int32_t flags,
                         void* workspace, size_t workspace_bytes,
                         ttx_stream_t stream);

/* ------------------------------ row cache over several tables (not in the reference) -----
 * The reference's cache serves one table (tt_embeddings_ops.py:456), and so do the entry points above.  For the num_tables
 * tables of ONE row shape of a table-batched bag (no p_tables) a single hashtbl / cache_freq / cache_state / cache_weight set is
 * keyed by
 *
 *   key = table * key_stride + index,   key_stride = prod(p) (>= num_embeddings: the range the index decode covers)
 *
 * so that the cache_size hottest rows ACROSS the tables are cached.  Every cache entry point above then works unchanged on
 * keys in place of indices and on the output / gradient viewed as [num_tables * B, D] (bags addressed by their flat row
 * table * B + b): ttx_update_cache_state, ttx_preprocess_indices_async called with num_tables = 1 and nb = num_tables * B
 * bags (its part_rowidx is then the flat bag row), ttx_cache_forward_n, ttx_cache_backward_*_n, ttx_cache_backward_sorted.
 * These three calls carry (table, index) into and out of key space and fill the cache rows:
 *
 *   ttx_table_keys        keys[n] = indices[n] + t(n) * key_stride, t(n) = the table whose extent
 *                         [offsets[t B], offsets[(t + 1) B]) holds position n.  offsets: the batch's num_tables * B + 1 bag
 *                         offsets, table-major, offsets[0] = 0 and the closing entry = nnz as everywhere; tables without
 *                         lookups (equal boundaries) and empty bags are legal; t(n) always lies in [0, num_tables - 1].  With
 *                         upd_hashtbl / upd_cache_freq (both or neither; H slots) the launch also counts the keys, exactly as
 *                         ttx_update_cache_state would.  One thread per lookup searches the num_tables + 1 table boundaries
 *                         (staged in LDS up to 1024 of them, read from the offsets beyond: no cap on num_tables), 64-bit
 *                         arithmetic throughout (key_stride may exceed 2^32).  One launch, one writer per element.
 *   ttx_table_keys_split  the inverse on the first *n_dev entries (a device int32, clamped to [0, n]; NULL: all n).
 *                         bagrow != NULL (the part_rowidx of the live preprocess, flat bag rows): t = bagrow[s] / B,
 *                         out_rowidx[s] = bagrow[s] - t B, out_indices[s] = keys[s] - t key_stride, out_tableidx[s] = t --
 *                         what ttx_plan_build_n takes for the misses.  bagrow == NULL: t = keys[s] / key_stride and
 *                         out_rowidx is not written (may be NULL).  t is clamped to [0, num_tables - 1] before it scales
 *                         anything.  Entries at and beyond the count are NOT written (a counted plan does not read them).
 *   ttx_cache_populate_t  ttx_cache_populate_f for a geometry with num_tables >= 1: the same sort and mark on the keys, the
 *                         cache_size selected keys split (bagrow == NULL) and decompressed by ttx_tt_rows with their
 *                         tables; an empty slot among them is row 0 of table 0.  key_stride <= prod(p).  Honours
 *                         TTX_POPULATE_REFERENCE_EXACT.  One 8-byte read-back sizes the sort, as in ttx_cache_populate.
 *   nnz == 0 / n == 0     returns 0 and launches nothing.
 *   errors                a negative size, nnz >= 2^31, B <= 0, num_tables <= 0, key_stride <= 0, num_tables * B >= 2^31,
 *                         num_tables * key_stride >= 2^62, counting with one of the two tables missing or H outside
 *                         (0, 2^31), an int64 pointer not 8-byte (n_dev: 4-byte) aligned, a NULL pointer that would be read
 *                         or written: -1 with ttx_last_error() set, before anything touches a device.
 * Nothing is read back by the first two (capturable); no atomics except the frequency count's. */
int ttx_table_keys(int64_t nnz, const int64_t* indices, int32_t num_tables, int64_t B, const int64_t* offsets,
                   int64_t key_stride, int64_t* keys, int64_t H, int64_t* upd_hashtbl, int64_t* upd_cache_freq,
                   ttx_stream_t stream);
int ttx_table_keys_split(int64_t n, const int32_t* n_dev, int32_t num_tables, int64_t B, int64_t key_stride,
                         const int64_t* keys, const int64_t* bagrow, int64_t* out_indices, int64_t* out_tableidx,
                         int64_t* out_rowidx, ttx_stream_t stream);
size_t ttx_cache_populate_t_workspace_bytes(const ttx_geom* g, int64_t hashtbl_size, int64_t cache_size, int32_t D);
int ttx_cache_populate_t(const ttx_geom* g, const float* const* tt_cores, int64_t hashtbl_size, int64_t* hashtbl,
                         int64_t* cache_freq, int32_t* cache_state, int64_t cache_size, int32_t D, float* cache_weight,
                         int64_t key_stride, int32_t flags, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ------------------------------ row cache over tables of different row factors (not in the reference) -----
 * The same ONE cache for the tables of a p_tables geometry (tables of different row factors, common q and ranks;
 * num_tables <= TTX_MAX_TABLES_MIXED).  A single stride no longer separates the tables: table k covers
 * stride_k = prod_t p_tables[k][t] rows, and a lookup (table k, index i) is the key
 *
 *   key = key_base[k] + i,   key_base[k] = sum_{j < k} stride_j,   key_base[num_tables] = the total
 *
 * The ranges are disjoint because i < num_embeddings_k <= stride_k.  key_base is a HOST array of num_tables + 1 int64, read
 * during the call only (as p_tables is): it travels in the kernel arguments -- no call below allocates device memory or copies
 * from pageable host memory, the first two read nothing back and are capturable in a hipGraph.  Everything said above about
 * keys in place of indices and bags addressed by their flat row holds unchanged.
 *
 *   ttx_table_keys_v        keys[n] = indices[n] + key_base[t(n)], t(n) found exactly as ttx_table_keys finds it: the last
 *                           of the num_tables + 1 table boundaries offsets[t B] that is <= n (empty tables and empty bags are
 *                           legal, t(n) always lies in [0, num_tables - 1]).  64-bit arithmetic throughout.  With
 *                           upd_hashtbl / upd_cache_freq (both or neither; H slots) the launch also counts the keys, exactly
 *                           as ttx_update_cache_state would.  One launch, one writer per element.
 *   ttx_table_keys_split_v  the inverse on the first *n_dev entries (a device int32, clamped to [0, n]; NULL: all n).
 *                           bagrow != NULL: t = bagrow[s] / B clamped to [0, num_tables - 1] before it indexes anything,
 *                           out_rowidx[s] = bagrow[s] - t B, out_indices[s] = keys[s] - key_base[t], out_tableidx[s] = t.
 *                           bagrow == NULL (populate): t = the last k in [0, num_tables - 1] with key_base[k] <= keys[s] (a
 *                           binary search of at most 6 steps; tables of stride 1 are found like any other) and out_rowidx is
 *                           not written (may be NULL).  Entries at and beyond the count are NOT written.
 *   ttx_cache_populate_v    ttx_cache_populate_t for a geometry that carries p_tables; key_base is derived from it on the
 *                           host.  The same sort and mark on the keys, the cache_size selected keys split (bagrow == NULL)
 *                           and decompressed by ttx_tt_rows on the p_tables geometry, each from its own table; an empty slot
 *                           among them is row 0 of table 0.  Honours TTX_POPULATE_REFERENCE_EXACT.  T == 3 only (the rows
 *                           route on per-table row factors has only ever run with three cores): any other T returns
 *                           TTX_EUNSUPPORTED.  One 8-byte read-back sizes the sort, as in ttx_cache_populate; a geometry seen
 *                           for the first time places its per-table factors on the device (as in every p_tables call).
 *   nnz == 0 / n == 0       returns 0 and launches nothing.
 *   errors                  a negative size, nnz >= 2^31, B <= 0, num_tables outside [1, TTX_MAX_TABLES_MIXED],
 *                           num_tables * B >= 2^31, key_base NULL, not starting at 0, not strictly increasing or ending at or
 *                           above 2^62, counting with one of the two tables missing or H outside (0, 2^31), an int64 pointer
 *                           not 8-byte (n_dev: 4-byte) aligned, a NULL pointer that would be read or written: -1 with
 *                           ttx_last_error() set, before anything touches a device. */
int ttx_table_keys_v(int64_t nnz, const int64_t* indices, int32_t num_tables, int64_t B, const int64_t* offsets,
                     const int64_t* key_base, int64_t* keys, int64_t H, int64_t* upd_hashtbl, int64_t* upd_cache_freq,
                     ttx_stream_t stream);
int ttx_table_keys_split_v(int64_t n, const int32_t* n_dev, int32_t num_tables, int64_t B, const int64_t* key_base,
                           const int64_t* keys, const int64_t* bagrow, int64_t* out_indices, int64_t* out_tableidx,
                           int64_t* out_rowidx, ttx_stream_t stream);
size_t ttx_cache_populate_v_workspace_bytes(const ttx_geom* g, int64_t hashtbl_size, int64_t cache_size, int32_t D);
int ttx_cache_populate_v(const ttx_geom* g, const float* const* tt_cores, int64_t hashtbl_size, int64_t* hashtbl,
                         int64_t* cache_freq, int32_t* cache_state, int64_t cache_size, int32_t D, float* cache_weight,
                         int32_t flags, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ------------------------------ cache refresh: trained rows across a re-populate (not in the reference) -----
 * Every populate above decompresses all cache_size rows anew, so what the cached rows learnt since the last populate is lost,
 * and the rows' optimizer state stays where it was while the keys change rows.  ttx_cache_carry runs AFTER any of the populates
 * (with flags = 0) and puts both where they belong, given copies of cache_state / cache_weight / the state taken BEFORE it.
 *
 *   per hash slot s in [0, hashtbl_size):  k = hashtbl[s], n = cache_state[s], m = old_state[s].  The slot takes part iff
 *       k != -1,  0 <= n < cache_size,  and  s is the slot the library's own probe finds k in (3 probes).
 *     (The last condition: a key can sit in two slots of its probe window -- an eviction emptied an earlier slot, a later count
 *      re-inserted the key there -- and the later copy then carries a stale cache_state that may name a row another key owns
 *      by now.  Only the findable copy owns its row.)
 *   kept      (0 <= m < cache_size):  cache_weight[n, :] = old_weight[m, :],  opt_state[n, :] = old_opt_state[m, :]
 *   admitted  (otherwise):            cache_weight[n, :] stays what the populate decompressed,  opt_state[n, :] = 0
 *   Rows that no participating slot owns are not written.
 *
 * state_width: 0 = no optimizer state (both state pointers are ignored), 1 = one float per row (row-wise Adagrad),
 * D = one per element; the state arrays are [cache_size, state_width].  One writer per row by construction: no atomics, no
 * read-back (capturable), bit-deterministic.  One launch: the slots are scanned with coalesced reads, a row is moved by a group
 * of lanes with 16-byte accesses when D % 4 == 0 and the row arrays are 16-byte aligned, float by float otherwise.
 *   cache_size == 0   returns 0 and launches nothing.
 *   errors            hashtbl_size outside (0, 2^31), cache_size < 0 or > hashtbl_size, D <= 0, state_width not in {0, 1, D},
 *                     hashtbl not 8-byte (any other pointer: 4-byte) aligned, a NULL pointer that would be read or written,
 *                     old_weight overlapping cache_weight or old_opt_state overlapping opt_state (the move is a permutation:
 *                     it cannot be done in place): -1 with ttx_last_error() set, before anything touches a device. */
int ttx_cache_carry(int64_t hashtbl_size, const int64_t* hashtbl, const int32_t* old_state, const int32_t* cache_state,
                    int64_t cache_size, int32_t D, const float* old_weight, float* cache_weight, int32_t state_width,
                    const float* old_opt_state, float* opt_state, ttx_stream_t stream);

/* replaces cache_forward_cuda (tt_embeddings.cpp:97-103,
 * tt_embeddings_cuda.cu:1498-1572): output[rowidx[n], :] += cache_weight[
 * cache_locations[n], :], summed per run of equal rowidx. */
int ttx_cache_forward(int32_t B, int64_t nnz, const int32_t* cache_locations,
                      const int64_t* rowidx, int32_t D,
                      const float* cache_weight, float* output,
                      ttx_stream_t stream);

/* replaces cache_backward_sgd_cuda (tt_embeddings.cpp:105-111,
 * tt_embeddings_cuda.cu:1574-1657):
 * cache_weight[loc[n], :] += -grad_output[rowidx[n], :] * lr. */
int ttx_cache_backward_sgd(int64_t nnz, int32_t D, const float* grad_output,
                           const int32_t* cache_locations, const int64_t* rowidx,
                           float learning_rate, float* cache_weight,
                           ttx_stream_t stream);

/* replaces cache_backward_dense_cuda (tt_embeddings.cpp:113-119,
 * tt_embeddings_cuda.cu:1659-1733): grad_cache_weight[cache_size, D] is
 * overwritten with the scatter-sum of grad_output rows. */
int ttx_cache_backward_dense(int64_t nnz, int32_t D, const float* grad_output,
                             const int32_t* cache_locations,
                             const int64_t* rowidx, int64_t cache_size,
                             float* grad_cache_weight, ttx_stream_t stream);

/* replaces cache_backward_rowwise_adagrad_approx_cuda (tt_embeddings.cpp:121-129,
 * tt_embeddings_cuda.cu:1735-1835): per bag g2 = mean(g*g); per cached lookup
 * old = state[loc] (then state[loc] += g2), w[loc,:] -= g * lr/(sqrt(old+g2)+eps).
 * Bags are processed in order (the reference leaves the order of two bags that
 * hit the same cache row to the hardware). */
int ttx_cache_backward_rowwise_adagrad_approx(
    int64_t nnz, int32_t D, const float* grad_output,
    const int32_t* cache_locations, const int64_t* rowidx, float learning_rate,
    float eps, float* cache_optimizer_state, float* cache_weight,
    ttx_stream_t stream);

/* ------------------------------------------------------------- profiling ---
 * Live kernel timing for bench.py's roofline block: ttx_profile_enable(mask)
 * selects kernel slots (bit w = slot w, 0 = off); every launch of a selected
 * kernel is bracketed by two HIP events on the launch stream.
 * ttx_profile_read synchronises the pending events and returns, for kernel
 * `which` (0 = forward contraction, 1 = backward contraction, 2 = reduce/apply,
 * 3 = plan, 4 = bag pooling, 5 = cache gather fwd), the launch count and the
 * summed duration in milliseconds since the last reset. */
#define TTX_PROF_FWD 0
#define TTX_PROF_BWD 1
#define TTX_PROF_APPLY 2
#define TTX_PROF_PLAN 3
#define TTX_PROF_POOL 4
#define TTX_PROF_CACHE_FWD 5
#define TTX_PROF_NUM 6
int ttx_profile_enable(int mask);
/* the same without reading back pending event pairs: for launches recorded inside a hipGraph capture, whose
 * events only carry times once the graph has been replayed (read them with ttx_profile_read afterwards) */
int ttx_profile_mask(int mask);
int ttx_profile_reset(void);
int ttx_profile_read(int which, int64_t* launches, double* total_ms);

/* The cache rows' update of one batch WITHOUT atomics: deterministic (bit-identical from run to run), one writer per cache row.
 * Replaces cache_backward_sgd_cuda / cache_backward_dense_cuda / cache_backward_rowwise_adagrad_approx_cuda
 * (tt_embeddings.cpp:105-129, tt_embeddings_cuda.cu:1574-1835) for callers that give it a workspace: the cached lookups
 * [*skip_dev, nnz) (skip_dev NULL: all) are grouped by cache row with a stable sort, a row's bag gradients are added in INDEX
 * order and applied once.  optim: TTX_OPTIM_SGD (dst = cache_weight, += -lr * sum), TTX_OPTIM_DENSE (dst = the cache_weight gradient
 * [cache_size, D], zeroed here) or TTX_OPTIM_ADAGRAD (dst = cache_weight, cache_optimizer_state [cache_size]: the reference's
 * per-lookup sequence old = state, state += g2, w -= g * lr / (sqrt(old + g2) + eps), taken in index order within a row -- the
 * order of a sequential execution, where the reference's depends on which warp arrives first).  num_bags: rows of grad
 * (row-wise Adagrad).  Up to 32,768 lookups (D % 4 == 0, D <= 256) it is ONE launch -- every work-group owns the rows
 * row % G == g, finds and groups them in LDS -- and needs no workspace; beyond that a chain of ~16 launches (stable radix sort, run
 * heads, ordered sums, apply).
 * CONTRACT: what lies in front of the split point is not read.  For a lookup without a cache row -- n < *skip_dev, or
 * cache_locations[n] outside [0, cache_size) -- neither rowidx[n] nor any row of grad_output is dereferenced, on either route;
 * cache_locations[n] is read only for n >= *skip_dev.  The caller may leave rowidx[0, *skip_dev) unset.  rowidx[n] of a cached
 * lookup must lie in [0, num_bags) (not checked).  The atomic entry points above stay: one launch, faster below ~300k cached lookups (row-wise
 * Adagrad: ~60k). */
size_t ttx_cache_backward_sorted_workspace_bytes(int64_t nnz, int64_t num_bags, int32_t D);
int ttx_cache_backward_sorted(int32_t optim, int64_t nnz, const int32_t* skip_dev, int64_t num_bags, int32_t D,
                              const float* grad_output, const int32_t* cache_locations, const int64_t* rowidx,
                              float learning_rate, float eps, int64_t cache_size, float* cache_optimizer_state,
                              float* dst, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ---- dense member tables (csrc/ttx_dense.hip; not in the reference) --------------------------------------
 * Bags over UNCOMPRESSED tables: the small members of a mixed-cardinality module, for which a TT factorisation saves nothing.
 * weight [R, D] float32 row-major holds the tables' rows one table after the other: table k owns rows [row_base[k], row_base[k + 1]),
 * R = row_base[num_tables].  row_base is a HOST array of num_tables + 1 int64 read during the call (it travels in the kernel
 * arguments, as key_base does in ttx_table_keys_v); num_tables <= TTX_MAX_TABLES_MIXED.  The batch is the table-major form of the
 * batched modules: indices [nnz] int64, offsets [num_tables * B + 1] int64, bag b belongs to table b / B.
 * CONTRACT
 *   padding     a slot is padding when its index is negative (the merged batches' sentinel -1), or when padding != NULL and the
 *               index equals padding[table] (HOST array, num_tables int64, a negative entry: the table has none).  Every other
 *               index is clamped into [0, E_k - 1] before it addresses anything: another row, never out of bounds.
 *   forward     mode 0 sum (per_sample_weights optional), 1 mean (divisor = the bag's count of non-padding slots, left in
 *               live[bag]), 2 max (strict > in position order: the first position wins a tie; argmax [num_tables * B, D] = the
 *               winning position n, -1 for a bag without a live slot -- as ttx_bag_max_pool).  A bag without a live slot gives
 *               zeros.  Every output element has one writer: no memset in front.
 *   backward    row r's gradient G_r = sum over r's live lookups n, in index order, of c_n * grad_output[bag(n)] (sum: the weight;
 *               mean: 1 / live; max: column e counts where argmax[bag(n), e] == n), lists longer than the split length of
 *               ttx_dense_bags_info summed per chunk and the chunk sums added in chunk order.  Applied ONCE per touched row:
 *               TTX_OPTIM_SGD w -= lr G; TTX_OPTIM_ADAGRAD with state_width == D (opt_state [R, D]) s += G^2, w -= lr G / (sqrt(s) + eps);
 *               with state_width == 1 (opt_state [R]) s_r += mean_e(G_e^2), w -= lr G / (sqrt(s_r) + eps); TTX_OPTIM_DENSE
 *               (state_width 0) d_weight[r] = G_r and zeros for every other row (the call writes every element of d_weight).
 *               d_per_sample_weights (NULL or [nnz], mode 0): <grad_output[bag(n)], weight[row(n)]> from the weights as they were
 *               BEFORE this call's update, 0 at padding.  No float atomics, one writer per row: bit-identical from run to run.
 *   paths       16-byte accesses when D % 4 == 0 and every float / int32 pointer is 16-byte aligned, a scalar path otherwise;
 *               rows wider than 256 floats are walked per column block; offsets are 64-bit.
 *   capture     nothing is read back to the host, nothing is allocated: both calls are capturable.
 *   errors      -1 with ttx_last_error() set, before anything touches a device: a negative size, nnz or num_tables * B >= 2^31,
 *               num_tables outside [1, TTX_MAX_TABLES_MIXED], row_base NULL / not starting at 0 / not strictly increasing,
 *               D <= 0, state_width not in {0, 1, D} or not matching optim, weights with a mode other than 0, argmax / live
 *               missing where the mode needs it, a NULL or misaligned pointer that would be used; TTX_EWORKSPACE for a workspace
 *               that is too small.  nnz == 0 still writes the zero output (and d_weight under DENSE) and trains nothing.
 * ttx_dense_bags_info (host-side, stateless): out[2] = {the list length beyond which a row's lookups are split into chunks of
 * that length, the batch size at which a one-launch route hands over -- 0: there is none, every batch takes the sorted route}. */
int ttx_dense_bags_forward(int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* offsets,
                           const int64_t* row_base, const int64_t* padding, const float* per_sample_weights, int32_t mode,
                           const float* weight, float* output, int32_t* live, int32_t* argmax, ttx_stream_t stream);
size_t ttx_dense_bags_backward_workspace_bytes(int64_t num_bags, int64_t nnz, int32_t D);
int ttx_dense_bags_backward(int32_t optim, int32_t num_tables, int64_t B, int32_t D, int64_t nnz, const int64_t* indices,
                            const int64_t* offsets, const int64_t* row_base, const int64_t* padding,
                            const float* per_sample_weights, int32_t mode, const int32_t* live, const int32_t* argmax,
                            const float* grad_output, float lr, float eps, int32_t state_width, float* opt_state, float* weight,
                            float* d_weight, float* d_per_sample_weights, void* workspace, size_t workspace_bytes,
                            ttx_stream_t stream);
int ttx_dense_bags_info(int32_t D, int64_t nnz, int32_t* out);

/* ---- fused Adam (csrc/ttx_adam.hip; not in the reference) -------------------------------------------------
 * One call is ONE optimizer step of torch.optim.Adam / AdamW (no amsgrad) over up to TTX_ADAM_MAX_TENSORS dense float32 tensors:
 * the cores of a TT module (their dense gradients from the TTX_OPTIM_DENSE routes), or the weight of a dense group.  Every
 * element steps, whatever its gradient.  numel, w, g, m, v are HOST arrays of ntensors entries (sizes, and device pointers to
 * weights, gradients, exp_avg, exp_avg_sq) read during the call: they travel in the kernel arguments.  step is a DEVICE int64 [1],
 * the number of steps taken so far.
 * CONTRACT
 *   update      with t = *step + 1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (in double), per element: decoupled != 0 and
 *               weight_decay != 0: w *= 1 - lr wd first;  g' = g, or g + wd w when weight_decay != 0 and decoupled == 0;
 *               m = beta1 m + (1 - beta1) g';  v = beta2 v + (1 - beta2) g'^2;  w -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).
 *               After the call *step == t.  The tensors of a call must not overlap; g is only read.
 *   step        MECHANISM: a one-thread launch in front advances *step and leaves lr / bc1 and 1 / sqrt(bc2) in the workspace; the
 *               element launch reads those two floats only.  No work-group reads a step another one has advanced; nothing is read
 *               back, nothing allocated: capturable, and a replayed graph advances *step as eager calls do (lr and the other
 *               scalars are baked into a captured call).  Two launches per call.
 *   paths       16-byte accesses on the full chunks of a tensor whose four pointers are 16-byte aligned, scalars on its tail and
 *               on a misaligned tensor; grid capped at 2,048 work-groups, grid-stride beyond.  A zero-size tensor is legal.
 *   errors      -1 with ttx_last_error() set, before anything touches a device: ntensors outside [0, TTX_ADAM_MAX_TENSORS], a
 *               negative size, a NULL pointer that would be read, a pointer not 4-byte aligned (step: 8-byte), a beta outside
 *               [0, 1), eps < 0, a workspace smaller than ttx_adam_apply_workspace_bytes(ntensors).  ntensors == 0, or every size
 *               zero: returns 0, launches nothing and leaves *step alone (step and workspace may then be NULL). */
#define TTX_ADAM_MAX_TENSORS 16
size_t ttx_adam_apply_workspace_bytes(int32_t ntensors);
int ttx_adam_apply(int32_t ntensors, const int64_t* numel, float* const* w, const float* const* g, float* const* m,
                   float* const* v, int64_t* step, float lr, float beta1, float beta2, float eps, float weight_decay,
                   int32_t decoupled, void* workspace, size_t workspace_bytes, ttx_stream_t stream);

/* ---- bf16 inference forward (csrc/ttx_tt_bf16.hip; not in the reference) --------------------------------
 * Forward-only lookups of a TRAINED three-core table from bf16 copies of its cores: product 1 (core_0 x core_1) of a pivot
 * chunk's lookups runs on mfma_f32_16x16x32_bf16 with fp32 accumulation, the last core is contracted per lookup on the VALU
 * from the fp32 accumulators (x_0 is not rounded).  Nothing here trains, and no existing entry point changes.
 * SUPPORTED (ttx_tt_rows_bf16_supported: host-side, stateless, touches no device; any p, any num_tables, p_tables or not):
 *   T == 3, r1 <= 64 and r2 <= 64, q0 <= 16, q1 <= 64, q2 <= 8, and an x_0 tile of at least 16 rows of
 *   ld = q1 (r2 + 1) rounded up to q1 (mod 64) floats, plus 1 KiB of lookup records, within 128 KiB of LDS (a pass holds 64 rows
 *   where they fit, else 32 or 16; beside a 64-row tile the pass's core-2 slices are staged in LDS when that keeps the
 *   work-group within 40 KiB).
 *   Everything else (T = 2, T = 4, a rank above 64, ...) returns 0 here and TTX_EUNSUPPORTED from the pack and rows calls.
 * PACKED LAYOUT (owned by this library; all bf16, every slice a multiple of 16 bytes except core 2 with q2 <= 4: 8 bytes):
 *   K1p = r1 rounded up to 32 (the MFMA's K), N1 = q1 r2, N1p = N1 rounded up to 16, Q2P = 4 if q2 <= 4 else 8; padding is +0.
 *   core 0   [slices][q0][K1p]     element (a, k1) of a slice at a K1p + k1: the A fragment of row a, 8 k per lane, one 16-byte load
 *   core 1   [slices][N1p][K1p]    TRANSPOSED: column n = b r2 + k2 of the fp32 slice [r1][q1][r2] holds its K index contiguously
 *                                  at n K1p + k1: the B fragment of column n is one 16-byte load; columns N1 .. N1p - 1 are zero
 *   core 2   [slices][r2][Q2P]     element (k2, c) at k2 Q2P + c: the q2 factors of one k2 are one 8 / 16-byte load
 *   slices = num_tables * p[t] (p_tables: the sum over the tables, table after table), in the order of the fp32 core.
 *   ttx_tt_pack_bf16_elems(g, t) = slices * elements of a packed slice (0: not supported / bad t); allocate 2 bytes each,
 *   16-byte aligned.  ttx_tt_pack_bf16 is ONE elementwise launch: round to nearest even, bit for bit tensor.to(torch.bfloat16)
 *   (a tie goes to the even significand, the largest finite fp32 rounds to Inf, Inf stays, NaN becomes 0x7FC0, subnormals round
 *   like any other value: nothing is flushed).
 * ROWS  ttx_tt_rows_bf16: rows [nnz, D] float32, 16-byte aligned, rows[n, :] = the TT row of lookup n in the ORIGINAL lookup
 *   order, from packed_cores (a HOST array of 3 device pointers).  plan: a plan of ttx_plan_build (with or without bag rows) for
 *   the same geometry and batch; NULL: built in the workspace (ttx_tt_rows_bf16_workspace_bytes; indices / tableidx as for
 *   ttx_tt_rows).  With a plan neither indices, tableidx nor the workspace is read.  One work-group per pivot chunk of the plan,
 *   cores addressed by the plan's slice ids only (clamped to the slices there are) -- which is all a p_tables geometry needs.
 *   No atomics, one writer per row element: bit-identical from run to run; nothing read back, nothing allocated: capturable.
 *   nnz == 0 returns 0 and launches nothing.
 * POOL  ttx_bag_sum_pool: output[b, :] = rows[offsets[b], :] + rows[offsets[b] + 1, :] + ... in index order (fp32, starting
 *   from +0), b < nb; offsets [nb + 1] int64 (closing entry included), rows in lookup order with contiguous bags.  One writer per
 *   element, an empty bag gives zeros, any D: 16-byte accesses when D % 4 == 0 and both float pointers are 16-byte aligned, a
 *   scalar path otherwise.  nb == 0 returns 0 and launches nothing.  The mean is ttx_bag_mean_scale on top.
 * NUMERICS (inputs: the bf16 cores; c_t below are their exact values).  A product of two bf16 values is exact in fp32, so the
 *   only roundings are those of fp32 accumulation -- and, for an implementation that feeds x_0 to a second MFMA, ONE rounding of
 *   x_0 to bf16 (this build does not round x_0; the bound allows it).  Against the float64 chain product on the same cores:
 *     |err(row[a, b, c])| <= 2^-8 sum_k2 |x_0[(a), (b, k2)]| |c_2[k2, c]|  +  (r1 + r2 + 2) 2^-24 sum_{k1, k2} |c_0| |c_1| |c_2|
 *   (first term: the unit roundoff of an 8-bit significand on every x_0; second: r1 fp32 additions and r2 fused multiply-adds,
 *   each with relative error <= 2^-24 of the running sum of absolute values, to first order, with 2 units of slack).
 *   A pooled element: the sum of its rows' bounds plus len 2^-24 sum |row|.
 * ERRORS  -1 (TTX_EINVAL) with ttx_last_error() set, before anything touches a device (a p_tables geometry seen for the first
 *   time places its factors on the device first, as in every p_tables call): a bad geometry, D != prod(q), nnz < 0 or >= 2^31,
 *   NULL packed cores / rows, NULL indices without a plan, a pointer not 16-byte aligned (packed cores, rows), bag_sum_pool:
 *   nb < 0 or >= 2^31, D <= 0, a NULL pointer with nb > 0, floats not 4-byte / offsets not 8-byte aligned.  TTX_EWORKSPACE for a
 *   workspace that is too small (no plan given), TTX_EUNSUPPORTED for a shape ttx_tt_rows_bf16_supported rejects. */
int ttx_tt_rows_bf16_supported(const ttx_geom* g);
int64_t ttx_tt_pack_bf16_elems(const ttx_geom* g, int32_t t);
int ttx_tt_pack_bf16(const ttx_geom* g, int32_t t, const float* core_f32, void* packed, ttx_stream_t stream);
size_t ttx_tt_rows_bf16_workspace_bytes(const ttx_geom* g, int32_t D, int64_t nnz);
int ttx_tt_rows_bf16(const ttx_geom* g, int32_t D, int64_t nnz, const int64_t* indices, const int64_t* tableidx,
                     const void* const* packed_cores, float* rows, const void* plan, void* workspace, size_t workspace_bytes,
                     ttx_stream_t stream);
int ttx_bag_sum_pool(int64_t nb, int32_t D, const int64_t* offsets, const float* rows, float* output, ttx_stream_t stream);

/* test entry: the stable descending 64-bit radix sort of (key, value) pairs behind ttx_cache_populate, on its own
 * (what the reference asks of cub::DeviceRadixSort::SortPairsDescending, tt_embeddings_cuda.cu:1280-1308).  Stateless. */
size_t ttx_debug_sort_workspace_bytes(int64_t n);
int ttx_debug_sort_pairs_desc(int64_t n, const int64_t* keys, const int64_t* vals, int64_t* keys_out, int64_t* vals_out,
                              void* workspace, size_t workspace_bytes, ttx_stream_t stream);
/* host-side query, stateless: the walk the generic kernels take for geometry g:
 * out[6] = {lookups per chunk, q1 blocks per column pass, rows per K block, column passes, K blocks, LDS bytes};
 * all zero when a shape-specialised kernel takes the geometry (or nothing fits the LDS). */
int ttx_debug_tiles(const ttx_geom* g, int32_t* out);
/* Test / ablation knobs (skip kernel phases, force the generic kernels, LDS budget, chunk size, stamps): NOT in this library.
 * They exist in the test build of the same sources only (-DTTX_TEST_HOOKS -> libttx_hooks.so; include/ttx_test_hooks.h);
 * libttx.so compiles every knob as a constant at its default and exports no setter.  ttx_has_test_hooks() tells the builds
 * apart (0 = product); ttx_debug_state() is the bit mask of knobs away from their defaults -- always 0 in the product build;
 * bench.py refuses to time a library where it is not. */
int ttx_has_test_hooks(void);
int ttx_debug_state(void);
int ttx_cache_debug_state(void); /* (internal helper of the above) */

#ifdef __cplusplus
}
#endif
#endif /* TTX_H_ */
