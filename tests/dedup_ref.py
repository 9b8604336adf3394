"""A host reference of the duplicate-lookup route (csrc/ttx_plan.hip "duplicate lookups", csrc/ttx_tt.hip pool_gather* / gsum_*),
numpy only.  TEST INFRASTRUCTURE.

The map of a batch onto its DISTINCT (table, index) pairs is integer work with one right answer: a STABLE sort of the lookups by
their key, the run heads, and the inverse.  `expected_map` states that from the definition (csrc/ttx_internal.h, the `DedupMap`
comment); `carve` restates where carve_dedup puts the arrays; `route` restates the ORDER OF CHOICES of the host code (the map's
two forms, the template argument and passes of the one, the passes and blocks of the other, whether tstart is written, the
pooling kernel, the pre-sum's vector type); `gsum_layout` says which kernel finishes each run of occurrences; `presum64` is the
pre-sum itself in float64.  The constants below mirror the library's; tests/test_dedup_routes_cpu.py reads the sources and fails
when one of them is retuned without this file.

Not restated: tables of different row factors (Dims::tab) -- dedup_supported refuses them, no map is built."""
import numpy as np

# ---- mirrors of the library's constants --------------------------------------------------------------------------------------
WAVE = 64                  # kWave
DEDUP_MAX_N = 16384        # kDedupMaxN: one work-group sorts the batch in LDS
PLAN_THREADS = 1024        # kPlanThreads (the small kernel's work-group); kPlanWaves = PLAN_THREADS / WAVE
PLAN_WAVES = PLAN_THREADS // WAVE
DD_THREADS = 1024          # kDdThreads: sorted positions per block of dd_count / dd_emit, block counts per trip of dd_scan
DD_BLOCK = 1024            # dedup_blocks: (nnz + 1023) / 1024
DEDUP_MAX_TABLES = 1023    # kDedupMaxTables: tstart has room for this many tables (+ 1)
DEDUP_HDR_BYTES = 64 + (DEDUP_MAX_TABLES + 1) * 8   # kDedupHdrBytes
TSTART_BYTE = 64           # dedup_tstart: (char*)M.nu + 64
ALIGN = 256                # align_up's default
BPW_LADDER = (2, 4, 8, 12, 16)   # dedup_small_kernel<BPW>: the first BPW with nb <= BPW
SMALL_KEY_BITS = 32        # dedup_key_space: tables * prod(p) <= 2^32 (and prod(p) <= 2^32) for the small form
SMALL_BITS_CAP = 32        # `while (bits < 32 && ...)` of dedup_build_map
LARGE_KEY_BITS = 61        # dedup_key_space64: tables * prod(p) <= 2^61
LARGE_BITS_CAP = 62        # `while (bits < 62 && ...)` of dedup_build_large
POOL_SPAN_MIN = 65536      # kPoolSpanMin: more lookups than this pool in pool_gather4_kernel
THREADS = 256              # kThreads (pooling work-groups)
GS_SLICE = 32              # kGsSlice: positions of the sorted occurrence list per 16-lane group
GS_FOLD_COOP = 64          # kGsFoldCoop: a run of more partials than this is folded by the whole work-group
GS_THREADS = 256           # kGsThreads: 16 groups = 16 slices per work-group
GS_GROUPS = GS_THREADS // 16
# plan_groups_tables (the plan's own constants, mirrored in tests/plan_ref.py too)
ONE_DIGIT = 256
WIDE_MAX_S = 4096
WIDE_SPAN = 4096           # kWideSpan
WIDE_MAX_G = 96            # kWideMaxG

SMALL, LARGE = 1, 2                                  # TTX_DD_SMALL / TTX_DD_LARGE
POOL_GATHER_VEC4, POOL_GATHER_SCALAR, POOL_SPAN = 1, 2, 3   # TTX_DD_POOL_*
VEC4, SCALAR = 1, 2                                  # TTX_DD_VEC4 / TTX_DD_SCALAR
ROUTE_FIELDS = ("form", "bpw", "passes", "nblk", "tstart", "pool", "gsum")   # tt_embeddings.DD_ROUTE_FIELDS


def r64(k):
    return (k + 63) // 64 * 64


def align_up(x, a=ALIGN):
    return (x + a - 1) // a * a


def rows_of(p):
    e = 1
    for x in p:
        e *= int(x)
    return e


# ---- the map -------------------------------------------------------------------------------------------------------------------
def keys_of(tables, p, indices, tableidx):
    """clamp(tableidx) * prod(p) + clamp(index), the clamps of dedup_small_kernel / dd_keys_kernel: a negative index is row 0, one
    >= prod(p) is the last row, the table goes into [0, tables - 1] (and is 0 when there is one table, whatever tableidx holds)"""
    E = rows_of(p)
    idx = np.clip(np.asarray(indices, dtype=np.int64), 0, E - 1)
    if tableidx is None or tables <= 1:
        tb = np.zeros_like(idx)
    else:
        tb = np.clip(np.asarray(tableidx, dtype=np.int64), 0, tables - 1)
    assert tables * E <= 1 << LARGE_KEY_BITS
    return tb * np.int64(E) + idx


def expected_map(tables, p, indices, tableidx):
    """every array of DedupMap -> dict(nu, uidx [nu], utab [nu], uid [nnz], occ [nnz], occ_off [nu + 1], iota [nnz], tstart [tables + 1],
    keys [nnz]).  The pairs are ascending by key on both forms; a pair's occurrences are in index order (the sorts are stable)."""
    E = rows_of(p)
    keys = keys_of(tables, p, indices, tableidx)
    nnz = keys.size
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    head = np.ones(nnz, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    starts = np.flatnonzero(head)
    nu = int(starts.size)
    ukey = sk[starts]
    uid = np.empty(nnz, dtype=np.int64)
    uid[order] = np.cumsum(head) - 1
    utab = ukey // E
    return dict(nu=nu, uidx=(ukey - utab * E).astype(np.int64), utab=utab.astype(np.int64), uid=uid.astype(np.int32),
                occ=order.astype(np.int32), occ_off=np.concatenate([starts, [nnz]]).astype(np.int32),
                iota=np.arange(nnz, dtype=np.int64), tstart=np.searchsorted(utab, np.arange(tables + 1), side="left").astype(np.int64),
                keys=keys)


def carve(nnz):
    """byte offsets of the map's arrays in the `dd` buffer (carve_dedup) -> dict(name: (byte offset, numpy dtype)), + "map_bytes"
    (dedup_map_bytes: where the large form's sort buffers begin)"""
    n = r64(nnz + 1)
    cur = 0
    lay = {"nu": (0, np.int32), "tstart": (TSTART_BYTE, np.int64)}
    cur += align_up(DEDUP_HDR_BYTES)
    for name in ("uidx", "utab", "iota"):
        lay[name] = (cur, np.int64)
        cur += align_up(n * 8)
    for name in ("uid", "occ", "occ_off"):
        lay[name] = (cur, np.int32)
        cur += align_up(n * 4)
    lay["map_bytes"] = cur
    return lay


# ---- the host-side choices -----------------------------------------------------------------------------------------------------
def _bits(all_keys, cap):
    bits = 1
    while bits < cap and (1 << bits) < all_keys:
        bits += 1
    return bits


def key_space32(tables, p):
    """dedup_key_space: tables * prod(p), or 0 when it (or prod(p)) is beyond 2^32"""
    E = rows_of(p)
    return tables * E if (E <= 1 << SMALL_KEY_BITS and tables * E <= 1 << SMALL_KEY_BITS) else 0


def key_space64(tables, p):
    """dedup_key_space64: tables * prod(p), or 0 beyond 2^61"""
    E = rows_of(p)
    return tables * E if (E <= 1 << LARGE_KEY_BITS and tables * E <= 1 << LARGE_KEY_BITS) else 0


def supported(tables, p, nnz):
    if nnz <= 0 or nnz >= 1 << 31:
        return False
    return (nnz <= DEDUP_MAX_N and key_space32(tables, p) != 0) or key_space64(tables, p) != 0


def small_nb(nnz):
    """64-position blocks per wave of dedup_small_kernel: per = ceil(N / 16) rounded up to a multiple of 64, nb = per / 64"""
    per = ((nnz + PLAN_WAVES - 1) // PLAN_WAVES + WAVE - 1) // WAVE * WAVE
    return per // WAVE


def plan_groups_tables(tables, p, nnz):
    """would the plan of the pairs sort each table group by itself (ttx_plan.hip plan_groups_tables)"""
    if tables <= 1:
        return False
    smax = tables * max(int(x) for x in p)
    if smax <= ONE_DIGIT:
        return False
    if smax <= WIDE_MAX_S and (nnz + WIDE_SPAN - 1) // WIDE_SPAN <= WIDE_MAX_G:
        return False
    return True


def route(tables, p, nnz, D, aligned=True, pool_aligned=None):
    """what ttx_dedup_build, ttx_tt_forward_dd and ttx_tt_backward_dd choose, as tt_embeddings.debug_dd_route reports it.
    aligned: d_output and the workspace's Gu on 16-byte addresses (the pre-sum's condition); pool_aligned: the workspace's rows and
    `output` (the pooling's; None = the same)."""
    assert supported(tables, p, nnz)
    pool_aligned = aligned if pool_aligned is None else pool_aligned
    r = dict.fromkeys(ROUTE_FIELDS, 0)
    if nnz > DEDUP_MAX_N or key_space32(tables, p) == 0:
        r.update(form=LARGE, bpw=0, passes=(_bits(key_space64(tables, p), LARGE_BITS_CAP) + 7) // 8, nblk=(nnz + DD_BLOCK - 1) // DD_BLOCK)
    else:
        nb = small_nb(nnz)
        r.update(form=SMALL, bpw=next(b for b in BPW_LADDER if nb <= b or b == BPW_LADDER[-1]),
                 passes=(_bits(key_space32(tables, p), SMALL_BITS_CAP) + 7) // 8, nblk=0)
    r["tstart"] = int(tables <= DEDUP_MAX_TABLES and plan_groups_tables(tables, p, nnz))
    if D % 4 == 0 and pool_aligned and nnz > POOL_SPAN_MIN:
        r["pool"] = POOL_SPAN
    elif D % 4 == 0 and pool_aligned:
        r["pool"] = POOL_GATHER_VEC4
    else:
        r["pool"] = POOL_GATHER_SCALAR
    r["gsum"] = VEC4 if (D % 4 == 0 and aligned) else SCALAR
    return r


def scan_trips(nnz):
    """trips of dd_scan_kernel's loop over the block counts (kDdThreads per trip): 2 from 1,048,577 lookups on"""
    nblk = (nnz + DD_BLOCK - 1) // DD_BLOCK
    return (nblk + DD_THREADS - 1) // DD_THREADS


# ---- the pre-sum ---------------------------------------------------------------------------------------------------------------
IN_SLICE, FOLD_ONE, FOLD_COOP = 0, 1, 2


def gsum_layout(occ_off, nnz):
    """for every run of occurrences (a distinct pair): dict(first, last: the slices of kGsSlice positions it begins / ends in; kind:
    IN_SLICE = finished by gsum_slice_kernel, FOLD_ONE = folded by the 16-lane group of its last slice, FOLD_COOP = more than
    kGsFoldCoop partials, folded by the 16 groups of that slice's work-group together; wg: the work-group of gsum_fold_kernel
    that finishes it)"""
    off = np.asarray(occ_off, dtype=np.int64)
    assert off[0] == 0 and off[-1] == nnz and (np.diff(off) > 0).all()
    first = off[:-1] // GS_SLICE
    last = (off[1:] - 1) // GS_SLICE
    span = last - first + 1
    kind = np.where(span == 1, IN_SLICE, np.where(span > GS_FOLD_COOP, FOLD_COOP, FOLD_ONE))
    return dict(first=first, last=last, kind=kind, wg=last // GS_GROUPS)


def presum64(m, rowidx, tableidx, B, d_out, per_sample_weights=None):
    """Gu[u] = sum over the occurrences n of pair u, IN occ ORDER, of w_n d_out[table(n), row(n)] in float64 -> [nu, D]
    (m: expected_map's dict)"""
    d = np.asarray(d_out, dtype=np.float64)
    d = d.reshape(-1, d.shape[-1])
    bag = np.asarray(tableidx, dtype=np.int64) * B + np.asarray(rowidx, dtype=np.int64)
    w = None if per_sample_weights is None else np.asarray(per_sample_weights, dtype=np.float64).reshape(-1)
    Gu = np.zeros((m["nu"], d.shape[1]))
    for u in range(m["nu"]):
        for k in range(int(m["occ_off"][u]), int(m["occ_off"][u + 1])):
            n = int(m["occ"][k])
            Gu[u] += d[bag[n]] if w is None else w[n] * d[bag[n]]
    return Gu


# ---- index sets from run layouts --------------------------------------------------------------------------------------------------
def pairs_from_counts(tables, p, counts, seed, spread=True):
    """distinct pairs in ascending key order, one per entry of `counts` -> (index [len], table [len]).  Since the map is sorted by
    key, counts ARE the run layout: run u covers positions [sum(counts[:u]), + counts[u]) of the sorted occurrence list.
    spread: the keys are drawn over the whole key space (every table gets its share), else they are the first ones."""
    E = rows_of(p)
    n = len(counts)
    assert n <= tables * E
    if spread:
        keys = np.sort(np.random.RandomState(seed).choice(tables * E, size=n, replace=False)) if tables * E <= 1 << 22 else \
            np.unique(np.random.RandomState(seed).randint(0, tables * E, size=4 * n + 16))[:n]
        assert keys.size == n
    else:
        keys = np.arange(n, dtype=np.int64)
    return (keys % E).astype(np.int64), (keys // E).astype(np.int64)
