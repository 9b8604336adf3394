"""A host mirror of the choices the four-core route makes on the host (csrc/ttx_tt.hip: t4_merge, t4_seg, t4_grid, t4_lds, the
helper dispatch of tt_backward_impl, t4_apply23_kernel's launch geometry) and the case table of tests/test_t4_routes_gpu.py.
TEST INFRASTRUCTURE: plain Python, no device.  tests/test_t4_routes_cpu.py reads the sources and fails when one of the mirrored
expressions changes without this file, and holds the case table against the mirror: every value of every field of route() is
taken by some case.  Whether the route is taken at all is tests/spec_ref.py's t4_merged.

A four-core lookup runs as: the merge (M = core_2[i_2] core_3[i_3] per lookup: t4_merge_sorted_kernel over `merge_seg` positions of
core 2's sorted order per work-group, or t4_merge_kernel per (lookup, row)), a three-core template on (core_0, core_1, M), and in
the backward a gradient helper (t4_grad23_mfma_kernel<Q3, 4 | 8> or t4_grad23_kernel<Q3, 8 | 16 | 32>) that leaves one partial
row of core 2 per run of SEG positions, then t4_apply23_kernel, which finds those rows at a slice's first position and at the
multiples of SEG inside it."""
import spec_ref as SR

T4_BATCH = 16          # kT4Batch: lookups the gradient helpers stage per step
T4_THREADS = 256       # kT4Threads
T4_APPLY_BLOCK = 1024  # kT4ApplyBlock = 4 * kT4Threads: elements of a core-2 slice per work-group of t4_apply23_kernel
T4_GRID_CAP = 16384    # t4_grid: at most this many work-groups of 256 (t4_merge_kernel strides beyond)
LDS_OPT_IN = 64 * 1024  # dynamic LDS above this needs allow_lds

SORTED, PER_LOOKUP = "sorted", "per_lookup"
HELPERS = ("mfma4", "mfma8", "valu8", "valu16", "valu32")
HELPER_ID = {h: i + 1 for i, h in enumerate(HELPERS)}   # TTX_T4_HELPER_* (include/ttx_test_hooks.h)
FORM_ID = {SORTED: 1, PER_LOOKUP: 2}                    # TTX_T4_MERGE_*
TEMPLATED = ("t4_merge_sorted_kernel", "t4_merge_kernel", "t4_grad23_kernel", "t4_grad23_mfma_kernel")


def seg(nnz):
    """t4_seg: positions of core 2's sorted order per work-group of the gradient helper = the stride of a slice's partial rows"""
    return 128 if nnz >= (1 << 18) else (64 if nnz >= (1 << 16) else (32 if nnz >= (1 << 14) else 16))


def merge_seg(nnz):
    """positions per work-group of t4_merge_sorted_kernel"""
    return 32 if nnz >= (1 << 17) else (16 if nnz >= (1 << 15) else 4)


def mfma_lds_floats(r2q2, r3, q3):
    """t4_lds(...).floats"""
    pm = r2q2 * q3
    pmS = pm + (2 * q3 - pm) % 32 if q3 in (2, 4, 8) else (pm + 3) // 4 * 4
    r3S = r3 + (16 - r3) % 32
    return r2q2 * r3S + T4_BATCH * pmS + T4_BATCH * r3 * q3


def core3_passes(n3):
    """t4_apply23_kernel's walk of a core-3 slice of n3 floats: [(V lanes per row, G row groups), ...], one entry per pass of e0"""
    out = []
    for e0 in range(0, n3, T4_THREADS):
        V = min(n3 - e0, T4_THREADS)
        out.append((V, T4_THREADS // V))
    return out


def route(q, ranks, nnz):
    """-> the record of a launch of nnz lookups of the four-core geometry (q, [r1, r2, r3]); None when it does not merge"""
    if SR.t4_merged(q, ranks) is None:
        return None
    q2, q3 = int(q[2]), int(q[3])
    r2, r3 = int(ranks[1]), int(ranks[2])
    r2q2 = r2 * q2
    n2, n3, pm = r2q2 * r3, r3 * q3, r2q2 * q3
    form = SORTED if (r3 <= 32 and r2q2 <= 256) else PER_LOOKUP
    mfma = r2q2 % 16 == 0 and r3 % 16 == 0 and n2 // 256 <= 32
    if mfma:
        helper = "mfma4" if n2 // 256 <= 16 else "mfma8"
        lds = 4 * mfma_lds_floats(r2q2, r3, q3)
    else:
        helper = "valu8" if n2 <= 8 * T4_THREADS else ("valu16" if n2 <= 16 * T4_THREADS else "valu32")
        lds = 4 * ((n2 + 3) // 4 * 4 + T4_BATCH * (pm + n3))
    template, pad = SR.match_any(q, ranks)
    return dict(
        merge=form,
        merge_seg=merge_seg(nnz) if form == SORTED else 0,
        merge_threads=(r2q2 + 63) // 64 * 64 if form == SORTED else 256,
        grid_wraps=form == PER_LOOKUP and (nnz * r2q2 + 255) // 256 > T4_GRID_CAP,
        SEG=seg(nnz),
        helper=helper,
        lds_bytes=lds,
        lds_opt_in=lds > LDS_OPT_IN,
        Q3=q3,
        n2=n2,
        n3=n3,
        nb2=(n2 + T4_APPLY_BLOCK - 1) // T4_APPLY_BLOCK,
        core3=core3_passes(n3),
        template=template,
        pad=pad,
    )


def kernels(rec):
    """the templated kernels a forward + backward of the record launches"""
    return ("t4_merge_sorted_kernel" if rec["merge"] == SORTED else "t4_merge_kernel",
            "t4_grad23_mfma_kernel" if rec["helper"].startswith("mfma") else "t4_grad23_kernel")


# ---- the case table of tests/test_t4_routes_gpu.py ---------------------------------------------------------------------------------
P4 = [4, 5, 3, 4]      # (a): 240 rows per table
SMALL_NNZ = 300        # about what a case of (a) launches: seg() = 16, merge_seg() = 4

# (a) name -> (q, [r1, r2, r3], the three-core template it merges onto, what the case is in the table for)
INSTANCES = {
    "mfma8_nb2_8": ([4, 4, 4, 2], [32, 32, 64], "S_32_4_32_8", "t4_grad23_mfma_kernel<2, 8>; eight blocks per core-2 slice"),
    "valu16": ([4, 4, 5, 3], [16, 24, 20], "S_32_8_32_16", "t4_grad23_kernel<3, 16>"),
    "valu32": ([4, 4, 5, 3], [16, 24, 40], "S_32_8_32_16", "t4_grad23_kernel<3, 32>"),
    "valu_lds": ([4, 4, 4, 8], [16, 30, 40], "S_32_4_32_32", "VALU helper with 101,120 B of dynamic LDS"),
    "mfma_lds_slice1024": ([4, 4, 2, 8], [16, 16, 128], "S_16_8_16_16", "MFMA helper above 64 KiB; core-3 slice of four whole passes"),
    "slice384": ([4, 4, 4, 8], [16, 16, 48], "S_16_4_16_32", "core-3 slice 384: passes of 256 and 128"),
    "slice300": ([4, 4, 3, 5], [16, 20, 60], "S_32_8_32_16", "core-3 slice 300: a remainder pass of 44 (G = 5, idle lanes)"),
    "q7_per_lookup_valu": ([4, 4, 4, 7], [16, 12, 33], "S_16_4_16_32", "Q3 = 7, per-lookup merge with r3 % 4 != 0"),
    "q7_sorted_mfma": ([2, 4, 4, 7], [16, 16, 16], "S_16_4_16_32", "Q3 = 7, sorted merge, MFMA"),
    "q1_per_lookup_valu": ([4, 4, 4, 1], [16, 12, 33], "S_16_4_16_4", "Q3 = 1, per-lookup merge, VALU"),
    "q1_sorted_mfma": ([2, 4, 4, 1], [16, 16, 16], "S2_16_4_16_4", "Q3 = 1, sorted merge, MFMA"),
    "q1_sorted_valu": ([4, 4, 4, 1], [16, 12, 9], "S_16_4_16_4", "Q3 = 1, sorted merge, VALU"),
    "q1_per_lookup_mfma": ([2, 4, 4, 1], [16, 16, 48], "S2_16_4_16_4", "Q3 = 1, per-lookup merge, MFMA"),
    # the rest of Q3 = 1 .. 8 under each of the four templated kernels: the smallest merging geometries
    "q2_sorted_mfma": ([2, 2, 2, 2], [16, 16, 16], "S2_16_2_16_4", "Q3 = 2"),
    "q2_per_lookup_valu": ([2, 2, 2, 2], [16, 12, 33], "S2_16_2_16_4", "Q3 = 2"),
    "q2_sorted_valu": ([2, 2, 2, 2], [16, 16, 4], "S2_16_2_16_4", "Q3 = 2"),
    "q3_sorted_mfma": ([4, 4, 2, 3], [16, 16, 16], "S_16_4_16_8", "Q3 = 3"),
    "q3_per_lookup_mfma": ([4, 4, 2, 3], [16, 16, 48], "S_16_4_16_8", "Q3 = 3"),
    "q3_sorted_valu": ([4, 4, 2, 3], [16, 12, 9], "S_16_4_16_8", "Q3 = 3"),
    "q4_sorted_mfma": ([2, 4, 1, 4], [16, 16, 16], "S2_16_4_16_4", "Q3 = 4"),
    "q4_per_lookup_valu": ([2, 4, 1, 4], [16, 12, 33], "S2_16_4_16_4", "Q3 = 4"),
    "q4_sorted_valu": ([2, 4, 1, 4], [16, 16, 6], "S2_16_4_16_4", "Q3 = 4"),
    "q4_per_lookup_mfma": ([2, 4, 1, 4], [16, 16, 48], "S2_16_4_16_4", "Q3 = 4"),
    "q5_sorted_mfma": ([4, 4, 1, 5], [16, 16, 16], "S_16_4_16_8", "Q3 = 5"),
    "q5_per_lookup_valu": ([4, 4, 1, 5], [16, 12, 33], "S_16_4_16_8", "Q3 = 5"),
    "q5_sorted_valu": ([4, 4, 1, 5], [16, 16, 5], "S_16_4_16_8", "Q3 = 5"),
    "q5_per_lookup_mfma": ([4, 4, 1, 5], [16, 16, 48], "S_16_4_16_8", "Q3 = 5"),
    "q6_sorted_mfma": ([4, 4, 1, 6], [16, 16, 16], "S_16_4_16_8", "Q3 = 6"),
    "q6_per_lookup_valu": ([4, 4, 1, 6], [16, 12, 33], "S_16_4_16_8", "Q3 = 6"),
    "q6_sorted_valu": ([4, 4, 1, 6], [16, 16, 6], "S_16_4_16_8", "Q3 = 6"),
    "q6_per_lookup_mfma": ([4, 4, 1, 6], [16, 16, 48], "S_16_4_16_8", "Q3 = 6"),
    "q7_sorted_valu": ([4, 4, 1, 7], [16, 16, 7], "S_16_4_16_8", "Q3 = 7"),
    "q7_per_lookup_mfma": ([4, 4, 1, 7], [16, 16, 48], "S_16_4_16_8", "Q3 = 7"),
    "q8_sorted_mfma": ([4, 4, 1, 8], [16, 16, 16], "S_16_4_16_8", "Q3 = 8"),
    "q8_sorted_valu": ([4, 4, 1, 8], [16, 16, 6], "S_16_4_16_8", "Q3 = 8"),
}

# (c) the batch-size switches: name -> (q, [r1, r2, r3]); D = 16
SWITCH = {
    "sorted_mfma4": ([2, 2, 2, 2], [16, 16, 16]),
    "sorted_valu8": ([2, 2, 2, 2], [16, 16, 4]),
    "per_lookup_r2q2_32": ([2, 2, 2, 2], [16, 16, 48]),
}
SWITCH_K = (14, 15, 16, 17, 18)
SWITCH_P = [2, 2, 8, 5]   # eight core-2 slices for the designed runs, five core-3 slices
# (b) the run structure, on one geometry of each helper family at SEG = 16
STRUCT = ("q2_sorted_mfma", "q3_sorted_valu", "slice300")
STRUCT_P = [2, 2, 8, 5]
REUSE_NNZ = 1 << 15       # (d): the smallest batch with merge_seg() = 16


def run_counts(SEG, nnz=None):
    """lookups per core-2 slice (eight slices), in slice order = the order of the sorted positions: a run of SEG that begins at 0 and
    ends on a multiple of SEG; one lookup (begins on a multiple); SEG - 1 (ends on one); SEG + 1; none; 5 SEG + 3 (more than four
    partial rows behind the first: the apply's loop with four rows in flight); then, with nnz given, half of all lookups in one
    slice and the rest in the last -- otherwise two, which leaves a total that is no multiple of 16"""
    c = [SEG, 1, SEG - 1, SEG + 1, 0, 5 * SEG + 3]
    if nnz is None:
        return c + [2, 0]
    rest = nnz - sum(c) - nnz // 2
    assert rest > 0
    return c + [nnz // 2, rest]


def core3_counts(total, G, slices=5):
    """lookups per core-3 slice: one; none; at least 8 G + 1 (the eight-rows-in-flight loop of every row group and a remainder); the
    rest split over the others"""
    big = max(8 * G + 1, total // 3)
    rest = total - 1 - big
    assert rest >= slices - 3
    c = [1, 0, big] + [rest // (slices - 3)] * (slices - 3)
    c[-1] += rest - sum(c[3:])
    return c
