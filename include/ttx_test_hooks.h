/* ttx_test_hooks.h -- test / ablation knobs of libttx.  TEST BUILD ONLY.
 *
 * These entry points exist in libttx_hooks.so, the same sources as libttx.so compiled with -DTTX_TEST_HOOKS
 * (__graft_entry__.build()); the product library exports none of them and compiles every knob as a constant at its
 * default (tests/test_module_cpu.py::test_product_library_has_no_test_knobs).  The knobs are plain globals of the test
 * library -- not per stream, not thread-safe: parity tests of code paths small shapes would not reach (the generic kernels,
 * their block walk, odd chunk sizes) and A/B timing (scripts/ablate*.py, phase_times*.py).  The Python shim routes through
 * the test library only while a knob is away from its default (tt_embeddings.debug_skip / set_chunk / debug_lds_budget ...).
 */
#ifndef TTX_TEST_HOOKS_H
#define TTX_TEST_HOOKS_H
#include "ttx.h"
#ifdef __cplusplus
extern "C" {
#endif

/* tuning knob (bench A/B, tests): indices per work-group chunk; 0 = heuristic */
int ttx_set_chunk(int32_t indices_per_chunk);
/* LDS budget in bytes (<= 163840; 0 = that) of the generic kernels' tile search.  The generic contraction kernels walk a
 * core_1 slice in K blocks x column passes sized to the budget (csrc/ttx_tt_generic.inc), so a small budget drives small
 * shapes through the walk that ranks >= 80 need.  Set it before sizing workspaces / plans. */
int ttx_debug_lds_budget(int32_t bytes);
/* bit mask: bits 0..7 kernel phases to skip (results INVALID), bit 8 force the generic kernels, bits 9..12 leave out launches,
 * bit 15 shape-specialised kernels for exact shapes only; bit 16 reduce_apply with a work-group per small slice instead of a wave
 * per slice (round 6; results stay valid up to the order of addition); bit 17 plans built while it is set list the pivot's chunks
 * in slot order (one column) instead of dealing the slots column-major over 8 columns, one per XCD (the order is
 * performance only: results stay bit-identical); bit 18 the shape-specialised backward stores its partial gradients as 4-byte
 * non-temporal stores from products in the C/D layout, as before the 16-byte stores (results stay bit-identical);
 * bits 19..20 force the flavour of the 16-byte partial stores for every launch: 1 non-temporal, 2 write-through, 3 plain (timing
 * only: results stay bit-identical); bit 21 reduce_apply_kernel also for the small launches that reduce_apply_small_kernel takes
 * (results stay valid up to the order of addition).  0 = normal operation. */
int ttx_debug_skip(int32_t mask);
/* The kernel the LAST reduce + apply launch of this process was (a plain global of the test library, written by the backward's
 * host code): 0 = none yet, TTX_REDUCE_FULL = reduce_apply_kernel, TTX_REDUCE_SMALL = reduce_apply_small_kernel. */
#define TTX_REDUCE_FULL 1
#define TTX_REDUCE_SMALL 2
extern int ttx_debug_reduce_route;
/* What the host code of the four-core route (csrc/ttx_tt.hip: t4_merge, the helper dispatch of the backward, the launch of
 * t4_apply23_kernel) chose for the LAST launch of this process that took it (a plain global of the test library; zeros: none yet;
 * tests/t4_ref.py is the host mirror the tests compare it with).  The merge fields are written by the forward AND the backward
 * (both launch the merge), the others by the backward. */
#define TTX_T4_MERGE_FORM 0   /* TTX_T4_MERGE_SORTED = t4_merge_sorted_kernel, TTX_T4_MERGE_PER_LOOKUP = t4_merge_kernel */
#define TTX_T4_MERGE_SEG 1    /* positions per work-group of the sorted form; 0 for the per-lookup form */
#define TTX_T4_MERGE_GRID 2   /* work-groups of the merge launch */
#define TTX_T4_SEG 3          /* SEG the gradient helper was launched with */
#define TTX_T4_HELPER 4       /* TTX_T4_HELPER_* */
#define TTX_T4_LDS_BYTES 5    /* its dynamic LDS */
#define TTX_T4_LDS_OPT_IN 6   /* 1 = more than 64 KiB: the launch went through allow_lds */
#define TTX_T4_APPLY_SEG 7    /* SEG t4_apply23_kernel was launched with; 0 = the launch was left out */
#define TTX_T4_HELPER_Q3 8    /* the helpers' template argument Q3 */
#define TTX_T4_ROUTE_INTS 9
#define TTX_T4_MERGE_SORTED 1
#define TTX_T4_MERGE_PER_LOOKUP 2
#define TTX_T4_HELPER_MFMA4 1 /* t4_grad23_mfma_kernel<Q3, 4> */
#define TTX_T4_HELPER_MFMA8 2 /* t4_grad23_mfma_kernel<Q3, 8> */
#define TTX_T4_HELPER_VALU8 3 /* t4_grad23_kernel<Q3, 8> */
#define TTX_T4_HELPER_VALU16 4
#define TTX_T4_HELPER_VALU32 5
extern int ttx_debug_t4_route[TTX_T4_ROUTE_INTS];
/* What the host code of the duplicate-lookup route (csrc/ttx_plan.hip dedup_build / dedup_build_map / dedup_build_large,
 * csrc/ttx_tt.hip ttx_tt_forward_dd / gsum_launch_t) chose LAST in this process (a plain global of the test library; zeros:
 * none yet; tests/dedup_ref.py::route is the host mirror the tests compare it with).  The first five fields are written by
 * ttx_dedup_build, TTX_DD_POOL by ttx_tt_forward_dd, TTX_DD_GSUM by the gradient pre-sum of ttx_tt_backward_dd (and of the
 * sorted cache-row update, which launches the same two kernels). */
#define TTX_DD_FORM 0         /* TTX_DD_SMALL = dedup_small_kernel, TTX_DD_LARGE = the 64-bit key sort (dedup_build_large) */
#define TTX_DD_BPW 1          /* template argument of dedup_small_kernel (2, 4, 8, 12, 16); 0 for the large form */
#define TTX_DD_PASSES 2       /* 8-bit passes of the sort */
#define TTX_DD_NBLK 3         /* blocks of 1024 sorted positions of the large form (dd_count / dd_scan / dd_emit); 0 for the small form */
#define TTX_DD_TSTART 4       /* 1 = dedup_tstart_kernel was launched */
#define TTX_DD_POOL 5         /* TTX_DD_POOL_* */
#define TTX_DD_GSUM 6         /* TTX_DD_VEC4 = gsum_slice_kernel / gsum_fold_kernel<float4>, TTX_DD_SCALAR = <float> */
#define TTX_DD_ROUTE_INTS 7
#define TTX_DD_SMALL 1
#define TTX_DD_LARGE 2
#define TTX_DD_POOL_GATHER_VEC4 1   /* pool_gather_kernel<float4> */
#define TTX_DD_POOL_GATHER_SCALAR 2 /* pool_gather_kernel<float> */
#define TTX_DD_POOL_SPAN 3          /* pool_gather4_kernel */
#define TTX_DD_VEC4 1
#define TTX_DD_SCALAR 2
extern int ttx_debug_dd_route[TTX_DD_ROUTE_INTS];
/* A/B knob (scripts/bench_cache.py): 1 = ttx_cache_forward uses the one-group-per-lookup kernel for every D */
int ttx_debug_cache_fwd(int32_t lookup_groups);
/* (scripts/phase_times.py) device buffer receiving 16 int64 wall-clock stamps per backward work-group; NULL = off */
int ttx_debug_stamps(void* device_buffer);

/* ---- the lookup plan, as the tests see it (tests/test_plan_routes_gpu.py; no knob: neither changes what the library does) ---- */
/* Where carve_plan (csrc/ttx_plan.hip) puts every array of a plan of `nnz` lookups, in ints from the start of the buffer:
 * out[2 k] = offset, out[2 k + 1] = length of array k; k = TTX_PLAN_HDR .. TTX_PLAN_CNT, then per core t < TTX_MAX_CORES
 * TTX_PLAN_CORE0 + TTX_PLAN_PER_CORE * t + {0 sid, 1 perm, 2 ipos, 3 off, 4..6 scratch} (zeros for t >= T); behind the
 * pairs out[TTX_PLAN_LAYOUT_MC] = lookups per chunk, [+1] = max_chunks, [+2] = T, [+3] = ttx_plan_bytes.  The offsets are
 * carve_plan's own: the function calls it on a made-up base address. */
#define TTX_PLAN_HDR 0
#define TTX_PLAN_CHUNK_REC 1
#define TTX_PLAN_LREC 2
#define TTX_PLAN_LROW 3
#define TTX_PLAN_CHUNK_OFF 4
#define TTX_PLAN_CNT 5
#define TTX_PLAN_CORE0 6
#define TTX_PLAN_PER_CORE 7
#define TTX_PLAN_LAYOUT_MC 68
#define TTX_PLAN_LAYOUT_INTS 72
int ttx_debug_plan_layout(const ttx_geom* g, int64_t nnz, int64_t* out);
/* The route the LAST plan build of this process took (a plain global of the test library, set where plan_build,
 * plan_build_mb, plan_build_batches and prologue_launch choose); 0 = none yet. */
#define TTX_ROUTE_TINY 1            /* plan_small_kernel */
#define TTX_ROUTE_SINGLE 2          /* mb_single_kernel<false> */
#define TTX_ROUTE_SINGLE_PROLOGUE 3 /* mb_single_kernel<true>: the lookup prologue of one batch */
#define TTX_ROUTE_UNITS 4           /* mb_count / mb_scatter on wave units */
#define TTX_ROUTE_WIDE 0            /* + bits: one wide digit of 10 / 11 / 12 bits -> 10, 11, 12 */
#define TTX_ROUTE_GROUPED 10        /* + bits: a wide digit per table group -> 20, 21 */
#define TTX_ROUTE_MULTIPASS 30      /* + the number of 8-bit passes -> 31, 32, 33, 34 */
#define TTX_ROUTE_MULTIBATCH 40     /* several batches in one launch (ttx_lookup_prologue_multi, plan_build_batches) */
int ttx_debug_plan_route(void);

#ifdef __cplusplus
}
#endif
#endif
