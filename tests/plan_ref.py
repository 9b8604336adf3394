"""A host reference of the lookup plan (csrc/ttx_plan.hip), numpy only.  TEST INFRASTRUCTURE.

The plan is integer work with one correct answer: per core t the slice id of every lookup, a STABLE sort of the lookups by it, the
inverse of that sort, the slice offsets, and for the pivot core (core 1) the lookups in its sorted order with their other cores'
slice ids and bag rows.  `expected` states that from the definition (ttx_internal.h, the `Plan` comment); `route` restates the ORDER
OF CHOICES by which the library picks one of its ways of building it -- plan_build, plan_build_mb, prologue_fusable.  The
constants below mirror the library's; tests/test_plan_routes_cpu.py reads the sources and fails when one of them is retuned
without this file."""
import numpy as np

# ---- mirrors of the library's constants --------------------------------------------------------------------------------------
TINY_MAX_N = 1024          # plan_build: `nnz > 1024 || !d.idx32 || n_dev` leaves the tiny route
ONE_MAX_N = 16384          # kOneMaxN: the single launch
PRO_MAX_BAGS = 4096        # kProMaxBags: bags of the fused prologue
WIDE_SPAN = 4096           # kWideSpan = kWideThreads * kSB: positions per work-group of the wide / multi-pass plans
WIDE_MAX_G = 96            # kWideMaxG: work-groups of the wide plan (rows every scatter work-group reads)
MAX_GROUPS = 32            # kMaxGroups (== kMaxGroupsHost): table groups
MB_FUSE_U = 256            # kMbFuseU: wave units whose counts the scatter pass scans itself
UNIT_MAX = 4096            # `N > kMbFuseU * 4096`: beyond, the one-pass sort takes the multi-pass kernels
MAX_MULTI = 16             # kMaxMulti: batches per multi-batch launch
FULL_CHUNK_LIMIT = 1 << 18  # `N / MC < (1 << 18)`: finish_wide's packed full-chunk count
ONE_DIGIT = 256            # one 8-bit pass
WIDE_DIGITS = ((10, 1024), (11, 2048), (12, 4096))   # (bits, slice ids) of plan_build_wide<BITS, false>
GROUP_DIGITS = ((10, 1024), (11, 2048))              # ... of plan_build_wide<BITS, true>: group size x largest p
WAVE = 64

# route ids (include/ttx_test_hooks.h TTX_ROUTE_*)
TINY, SINGLE, SINGLE_PROLOGUE, UNITS = 1, 2, 3, 4
WIDE, GROUPED, MULTIPASS, MULTIBATCH = 0, 10, 30, 40   # WIDE + bits, GROUPED + bits, MULTIPASS + passes
WIDE10, WIDE11, WIDE12, GROUPED10, GROUPED11 = 10, 11, 12, 20, 21
ALL_ROUTES = (TINY, SINGLE, SINGLE_PROLOGUE, UNITS, WIDE10, WIDE11, WIDE12, GROUPED10, GROUPED11, MULTIPASS + 1, MULTIPASS + 2,
              MULTIPASS + 3, MULTIBATCH)
ONE_LAUNCH_COUNTS_PIVOT = (SINGLE, SINGLE_PROLOGUE, UNITS, MULTIBATCH)  # finish_single_pass: hdr[8 + 1] is a COUNT


def route_name(rid):
    names = {TINY: "tiny", SINGLE: "single", SINGLE_PROLOGUE: "single-as-prologue", UNITS: "units", MULTIBATCH: "multi-batch"}
    if rid in names:
        return names[rid]
    if MULTIPASS < rid < MULTIBATCH:
        return f"multi-pass x{rid - MULTIPASS}"
    if GROUPED + 10 <= rid <= GROUPED + 12:
        return f"grouped wide{rid - GROUPED}"
    return f"wide{rid - WIDE}"


def route_family(rid):
    """the coarse label of tests/fuzz_cases.py"""
    if rid in (SINGLE, SINGLE_PROLOGUE, MULTIBATCH):
        return "single"
    if WIDE10 <= rid <= WIDE12:
        return "wide"
    if GROUPED10 <= rid <= GROUPED11:
        return "table groups"
    if MULTIPASS < rid < MULTIBATCH:
        return "multi-pass"
    return route_name(rid)


class Geom:
    """tables of row factors p (one list, or one list per table), as the library's Dims sees them"""

    def __init__(self, tables, p):
        self.tables = int(tables)
        self.mixed = isinstance(p[0], (list, tuple, np.ndarray)) and self.tables > 1
        if isinstance(p[0], (list, tuple, np.ndarray)):
            pt = np.array([list(map(int, row)) for row in p], dtype=np.int64)
            if not self.mixed:
                pt = pt[:1]
        else:
            pt = np.array([list(map(int, p))] * self.tables, dtype=np.int64)
        assert pt.shape[0] == self.tables
        self.p_tables = pt                                              # [tables, T]
        self.T = pt.shape[1]
        self.S = [int(pt[:, t].sum()) for t in range(self.T)]
        self.base = [np.concatenate([[0], np.cumsum(pt[:, t])[:-1]]).astype(np.int64) for t in range(self.T)]
        self.p_max = [int(pt[:, t].max()) for t in range(self.T)]
        # (make_dims: tables of different row factors never decode in 32 bits)
        self.idx32 = (not self.mixed) and int(np.prod([int(x) for x in pt[0]])) <= 2 ** 32
        self.rows = [int(np.prod([int(x) for x in row])) for row in pt]  # prod(p) per table


def passes_of(S):
    bits = 0
    while (1 << bits) < S:
        bits += 1
    return max((bits + 7) // 8, 1)


def prologue_fusable(g, N, nb):
    return g.tables == 1 and TINY_MAX_N < N <= ONE_MAX_N and 1 <= nb <= PRO_MAX_BAGS and max(g.S) <= ONE_DIGIT


def group_shape(g, N):
    """(tables per group, groups, group size x largest p, count rows per group) of the table-group plan"""
    gsz = (g.tables + MAX_GROUPS - 1) // MAX_GROUPS
    ngroups = (g.tables + gsz - 1) // gsz
    return gsz, ngroups, gsz * max(g.p_max), N // WIDE_SPAN // ngroups + 1


def route(g, N, mc, n_dev=False, entry="build", nb=0):
    """the route id of a plan of N lookups (N sizes the buffers: with a device-side count it is the upper bound).
    entry: "build" (ttx_plan_build / _n), "prologue" (ttx_lookup_prologue: table-major offsets of nb bags),
    "multi" (ttx_lookup_prologue_multi, any number of batches: the id the LAST launch leaves).
    Not restated: plan_build_batches / plan_batches_ok, the cache-live prefetch of several batches (csrc/ttx_cache.hip) -- it launches
    the same mb_single_kernel<false> with grid.z = batch and sets the multi-batch id, but no test of the plan files drives it."""
    if entry in ("prologue", "multi") and prologue_fusable(g, N, nb):
        return MULTIBATCH if entry == "multi" else SINGLE_PROLOGUE
    offsets = entry in ("prologue", "multi")
    # plan_build
    if N <= TINY_MAX_N and g.idx32 and not n_dev:
        return TINY
    # plan_build_mb
    maxp = max(passes_of(s) for s in g.S)
    smax = max(g.S)
    if maxp == 1 and N <= ONE_MAX_N and not g.mixed:
        return SINGLE
    rows = (N + WIDE_SPAN - 1) // WIDE_SPAN
    if (maxp > 1 or g.mixed) and rows <= WIDE_MAX_G and N // max(mc, 1) < FULL_CHUNK_LIMIT:
        for bits, span in WIDE_DIGITS:
            if smax <= span:
                return WIDE + bits
    if offsets and g.tables > 1 and maxp > 1:
        _, _, span, grows = group_shape(g, N)
        if span <= GROUP_DIGITS[-1][1] and grows <= WIDE_MAX_G:
            return GROUPED + (GROUP_DIGITS[0][0] if span <= GROUP_DIGITS[0][1] else GROUP_DIGITS[1][0])
    if maxp > 1 or N > MB_FUSE_U * UNIT_MAX or g.mixed:
        return MULTIPASS + maxp
    return UNITS


def unit_positions(N):
    """positions per wave unit of the units route (mb_count / mb_scatter)"""
    unit = 256
    if (N + 255) // 256 > MB_FUSE_U:
        unit = ((N + MB_FUSE_U - 1) // MB_FUSE_U + WAVE - 1) // WAVE * WAVE
    return unit


def slice_ids(g, indices, tableidx):
    """[T] x int64[n]: sid[t][n] = first slice of the lookup's table in core t + i_t, with i_t = idx / L_t (% p_t behind core 0) of the
    table's own factors, CLAMPED as the library's decode clamps: a negative index is index 0, a factor beyond its range is the
    last one (decode_core / slice_id, csrc/ttx_plan.hip).  Indices from 2^32 on of a geometry with prod(p) <= 2^32 are left out
    of this statement: the tiny route saturates them to 2^32 - 1 before it decodes, the others decode them as they are."""
    idx = np.maximum(np.asarray(indices, dtype=np.int64), 0)
    tb = np.asarray(tableidx, dtype=np.int64)
    assert tb.size == idx.size and (tb.size == 0 or (tb.min() >= 0 and tb.max() < g.tables))
    assert not g.idx32 or idx.size == 0 or int(idx.max()) < 2 ** 32
    pt = g.p_tables[tb]                                                 # [n, T]
    out = []
    for t in range(g.T):
        L = np.prod(pt[:, t + 1:], axis=1) if t + 1 < g.T else np.ones(idx.size, dtype=np.int64)
        a = idx // L
        if t > 0:
            a = a % pt[:, t]
        out.append(g.base[t][tb] + np.minimum(a, pt[:, t] - 1))
    return out


def expected(g, indices, tableidx, rowidx, mc):
    """-> dict: n; sid, perm, ipos, off, lens: [T] arrays (perm = the STABLE argsort of sid, ipos its inverse, off[t][s] = first
    position of slice s, S_t + 1 entries); lrec [n, 4] = {lookup, sid_0, sid_2, sid_3} in the pivot core's sorted order (0 for a
    core the geometry does not have), lrow [n] = its bag row; nchunks = sum over the pivot's slices of ceil(len / mc); hot [T] =
    slices beyond reduce_apply's thresholds (thin cores: more than 512 lookups, pivot: more than 16 chunks)."""
    sid = slice_ids(g, indices, tableidx)
    n = int(np.asarray(indices).size)
    perm, ipos, off, lens = [], [], [], []
    for t in range(g.T):
        pm = np.argsort(sid[t], kind="stable")
        ip = np.empty(n, dtype=np.int64)
        ip[pm] = np.arange(n, dtype=np.int64)
        ln = np.bincount(sid[t], minlength=g.S[t]).astype(np.int64)
        perm.append(pm), ipos.append(ip), lens.append(ln)
        off.append(np.concatenate([[0], np.cumsum(ln)]).astype(np.int64))
    pv = perm[1]
    zero = np.zeros(n, dtype=np.int64)
    lrec = np.stack([pv, sid[0][pv], sid[2][pv] if g.T > 2 else zero, sid[3][pv] if g.T > 3 else zero], axis=1)
    lrow = np.asarray(rowidx, dtype=np.int64)[pv] if rowidx is not None else None
    rows1 = -(-lens[1] // int(mc))
    hot = [int((rows1 > HOT_PIVOT).sum()) if t == 1 else int((lens[t] > 2 * SEG_THIN).sum()) for t in range(g.T)]
    return dict(n=n, sid=sid, perm=perm, ipos=ipos, off=off, lens=lens, lrec=lrec, lrow=lrow, nchunks=int(rows1.sum()), hot=hot)


SEG_THIN = 256   # TTX_SEG_THIN   (tests/tt_ref64.py mirrors them too; tests/test_tt_ref64_cpu.py pins those to the sources)
HOT_PIVOT = 16   # TTX_HOT_PIVOT


def check_chunks(exp, mc, hdr0, chunk_rec, chunk_off):
    """The chunk list's invariants (its ORDER is a route's own): every record has 1 <= count <= mc; the chunks of slice
    s are the partial slots chunk_off[s] .. chunk_off[s + 1] - 1 and, taken in slot order, tile [off[1][s], off[1][s + 1]) without
    gap or overlap; the slots are distinct and inside [0, hdr0), what reduce_apply reads for hdr0 chunks.
    chunk_rec: [>= hdr0, 4] = {slice, start, count, slot}; chunk_off: [S_1 + 1].  Raises AssertionError."""
    off1, lens1 = exp["off"][1], exp["lens"][1]
    assert hdr0 == exp["nchunks"], f"hdr[0] = {hdr0}, sum of ceil(len / MC) = {exp['nchunks']}"
    rec = np.asarray(chunk_rec[:hdr0], dtype=np.int64)
    coff = np.asarray(chunk_off, dtype=np.int64)
    rows1 = -(-lens1 // int(mc))
    assert np.array_equal(coff, np.concatenate([[0], np.cumsum(rows1)])), "chunk_off is not the prefix sum of ceil(len / MC)"
    if hdr0 == 0:
        return
    s, start, cnt, slot = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    assert cnt.min() >= 1 and cnt.max() <= mc, f"a chunk of {cnt.min()} .. {cnt.max()} lookups (MC {mc})"
    assert s.min() >= 0 and s.max() < lens1.size, "a chunk of a slice the core does not have"
    assert np.array_equal(np.sort(slot), np.arange(hdr0)), "the partial slots are not a permutation of [0, hdr[0])"
    order = np.argsort(slot, kind="stable")
    s, start, cnt, slot = s[order], start[order], cnt[order], slot[order]
    assert np.array_equal(s, np.repeat(np.arange(lens1.size), rows1)), "a slice's slots are not chunk_off[s] .. chunk_off[s + 1] - 1"
    first = slot == coff[s]
    want = np.where(first, off1[s], np.concatenate([[0], (start + cnt)[:-1]]))
    assert np.array_equal(start, want), "the chunks of a slice leave a gap or overlap"
    last = slot == coff[s + 1] - 1
    assert np.array_equal((start + cnt)[last], off1[s[last] + 1]), "the chunks of a slice do not end where the slice ends"
