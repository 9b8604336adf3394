"""The duplicate-lookup route (dedup=True / "auto": csrc/ttx_plan.hip dedup_*, dd_*; csrc/ttx_tt.hip pool_gather*, gsum_*) at the
sizes that switch its kernels: the MAP array by array against a stable sort in numpy, the SUMS against float64.

Every case runs THROUGH THE TEST LIBRARY, which reports what the host code chose (ttx_debug_dd_route: the map's form, the
template argument, passes and blocks, whether tstart was written, the pooling kernel, the pre-sum's vector type); the record
must be what tests/dedup_ref.py::route expects.  tests/test_dedup_routes_cpu.py holds that mirror against the sources and this
file's case tables against the mirror (every value of every choice expected by a case, both sides of every threshold).

(a) test_map_arrays_and_route -- MAP_CASES.  A case is built twice into buffers pre-filled with different bytes; nu, uidx, utab,
uid, occ, occ_off, iota and tstart must EQUAL dedup_ref.expected_map (occ IS the stable argsort of the keys: an unstable sort,
which only changes the order of an fp32 sum, fails here), the two builds must be byte-identical on those ranges, and where tstart
is not written its bytes must still be the fill.  Sizes: 1, 63, 64, 65, the nb edges of the dedup_small_kernel<2|4|8|12|16>
ladder, 16384 | 16385 (one work-group <-> the 64-bit key sort); key spaces of 2^8, 2^8 + 1, 2^16, 2^16 + 1, 2^24, 2^24 + 1 and
exactly 2^32 keys (two tables of 2^31 rows, and one table of 2^32), beyond 2^32 at 100 lookups, and 1, 4, 5 and 8 passes of the
64-bit sort; streams: uniform with duplicates, one pair, all distinct, only the smallest and largest key of every table, indices
and tables equal only after the clamp, tables without a lookup, 40 tables in groups, kDedupMaxTables | + 1 tables; and
dd_scan_kernel's second trip (1,048,576 | 1,048,577 lookups, few pairs / a head in every block) -- map only.

(b) test_sums_end_to_end -- E2E_CASES, against tt_ref64.forward_backward.  Index sets are built from a list of COUNTS per pair in
key order: the map is sorted by key, so the counts are the layout of the runs over the pre-sum's slices of 32 positions
(dedup_ref.gsum_layout; the CPU file checks each layout has the runs its name says): inside a slice, ending on position 31, starting
on position 0, exactly a slice, whole slices inside a run, ending on a slice's last position after crossing, 64 | 65 | 66 slices (the
cooperative fold begins at 65), a cooperative and a short crossing run ending in one work-group, N < 32, N no multiple of 32 --
each at D = 16, 72, 128 (float4), 15, 18 (float), D = 16 with d_output off 16-byte alignment (float at D % 4 == 0), with
per_sample_weights, over three tables, on the specialised q = [4,4,4] r = [16,16] kernels.  Bag layouts for pool_gather_kernel
(lengths 0, 1, 15, 16, 17, 32, 33, leading and trailing empty bags) in float4 and float, and for pool_gather4_kernel at 65,537
lookups (64 one-lookup bags in a span, a span without a head, a bag from lane 63 running 81 lookups on, a bag from lane 0, the
last partial span) with 65,536 on the other side of kPoolSpanMin.
Per case: the forward bit-identical to the plain path and within tolerance of float64; dense gradients, fused SGD and fused
Adagrad FROM tt_ref64.live_state against float64; untouched slices bit-identical; a second run bit-identical.

Tolerance: the default of tests/util.py (rtol 1e-5, atol 2e-6 max|ref|) for EVERY comparison -- no case takes the widening rule
tt_ref64.widen_factor (the worst gradient here is 0.22 default bounds from float64, where the fp32 ORACLE, which adds a pair's
occurrences into one running sum, is up to 2.9 bounds away on the same cases).  profiles/dedup_tolerances.md holds the measured
distances and the record of three seeded mistakes these cases catch, one of which tests/test_dedup_gpu.py does not see.

Found: nothing.  The two places the issue named -- the small kernel at exactly 2^32 keys (ks-2^32-two-tables, ks-2^32-one-table:
the largest key 2^32 - 1 and the key 2^31, negative as the int the kernel keeps in LDS) and gsum_fold_kernel's choice of the
folding group for a run that ends on the last position of a slice (layout "edges": the run [104, 256)) -- compute what the
reference computes."""
import json
import os
import zlib

import numpy as np
import pytest
import torch

import dedup_ref as DR
import gen_inputs as G
import tt_ref64 as R
from util import EPS, LR, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

Q3, R3 = [2, 3, 2], [1, 4, 5, 1]           # generic and cheap (the plan tests' geometry)
P3 = [7, 6, 5]                             # 210 rows
P64 = [1700, 1700, 1700]                   # prod(p) > 2^32: never the small form
P2_31 = [2048, 1024, 1024]                 # 2^31 rows
P2_32 = [2048, 2048, 1024]                 # 2^32 rows: still the 32-bit decode
P2_60 = [1 << 20, 1 << 20, (1 << 20) - 1]  # just under 2^61 / 2
LADDER = (1, 63, 64, 65, 2048, 2049, 4096, 4097, 8192, 8193, 12288, 12289, 16384, 16385)
BASIC = ("uniform", "ends", "clamp")
ALL_STREAMS = ("uniform", "same", "distinct", "ends", "clamp", "empty_tables", "few", "heads")


def mcase(name, tables, p, N, streams):
    return dict(name=name, tables=tables, p=p, N=N, streams=tuple(streams))


MAP_CASES = [mcase(f"n-{n}", 1, P3, n, ("uniform",) + (("same", "ends", "clamp") if n in (65, 16384, 16385) else ())) for n in LADDER]
MAP_CASES += [
    mcase("distinct-65", 1, P3, 65, ("distinct",)),
    mcase("distinct-16384", 1, [32, 32, 64], 16384, ("distinct",)), mcase("distinct-16385", 1, [32, 32, 64], 16385, ("distinct",)),
    # ---- key spaces of the small form: 1 | 2 | 3 | 4 passes
    mcase("ks-2^8", 1, [4, 8, 8], 300, BASIC), mcase("ks-2^8+1", 1, [257, 1, 1], 300, BASIC),
    mcase("ks-2^16", 1, [32, 32, 64], 300, BASIC), mcase("ks-2^16+1", 1, [65537, 1, 1], 300, BASIC),
    mcase("ks-2^24", 1, [256, 256, 256], 300, BASIC), mcase("ks-2^24+1", 1, [257, 97, 673], 300, BASIC),
    mcase("ks-2^32-two-tables", 2, P2_31, 300, BASIC + ("same",)), mcase("ks-2^32-one-table", 1, P2_32, 300, BASIC + ("same",)),
    # ---- beyond 2^32 keys: the 64-bit sort at a small batch; its 1 (n-16385), 4, 5 and 8 passes
    mcase("ks-3x2^31", 3, P2_31, 100, BASIC), mcase("ks-64bit-100", 1, P64, 100, BASIC),
    mcase("large-4-passes", 1, [257, 97, 673], 16385, ("uniform", "ends")),
    mcase("large-8-passes", 2, P2_60, 100, BASIC),
    # ---- tables: tstart only when the plan of the pairs sorts table groups (plan_groups_tables) and tstart has room
    mcase("tables-3", 3, P3, 3000, ("uniform", "ends", "clamp")),
    mcase("tstart-7", 7, [700, 6, 5], 3000, ("uniform", "empty_tables", "ends", "clamp")),
    mcase("tstart-40", 40, [110, 6, 5], 3000, ("uniform", "empty_tables")),
    mcase("S-4096", 16, [256, 6, 5], 3000, ("uniform",)), mcase("S-4097", 17, [241, 6, 5], 3000, ("uniform",)),
    mcase("S-256", 4, [64, 6, 5], 3000, ("uniform",)), mcase("S-257-many-rows", 2, [200, 6, 5], 393217, ("uniform",)),
    mcase("S-257-few-rows", 2, [200, 6, 5], 393216, ("uniform",)),
    mcase("tables-1023", 1023, [5, 6, 5], 3000, ("uniform", "empty_tables")), mcase("tables-1024", 1024, [5, 6, 5], 3000, ("uniform",)),
    # ---- dd_scan_kernel: one trip of 1024 block counts | a second trip with a carry
    mcase("scan-1048576", 1, [256, 256, 256], 1 << 20, ("few", "heads")), mcase("scan-1048577", 1, [256, 256, 256], (1 << 20) + 1, ("few", "heads")),
]


def _rt(c, D=12, **kw):
    return DR.route(c["tables"], c["p"], c["N"], D, **kw)


def _one(c):
    return c["tables"] == 1 and c["p"] == P3


# (label, cases of the near side, what their route must hold, cases of the far side, theirs)
MAP_THRESHOLDS = [
    (f"N = {lo} | {lo + 1}: dedup_small_kernel<{b0}> <-> <{b1}>", (lambda c, lo=lo: _one(c) and c["N"] == lo), dict(form=DR.SMALL, bpw=b0),
     (lambda c, lo=lo: _one(c) and c["N"] == lo + 1), dict(form=DR.SMALL, bpw=b1))
    for lo, b0, b1 in ((2048, 2, 4), (4096, 4, 8), (8192, 8, 12), (12288, 12, 16))
] + [
    ("N = 16384 | 16385: one work-group <-> the 64-bit key sort", lambda c: _one(c) and c["N"] == 16384, dict(form=DR.SMALL, bpw=16, passes=1, nblk=0),
     lambda c: _one(c) and c["N"] == 16385, dict(form=DR.LARGE, bpw=0, passes=1, nblk=17)),
    ("2^8 | 2^8 + 1 keys", lambda c: c["name"] == "ks-2^8", dict(form=DR.SMALL, passes=1), lambda c: c["name"] == "ks-2^8+1", dict(form=DR.SMALL, passes=2)),
    ("2^16 | 2^16 + 1 keys", lambda c: c["name"] == "ks-2^16", dict(form=DR.SMALL, passes=2), lambda c: c["name"] == "ks-2^16+1", dict(form=DR.SMALL, passes=3)),
    ("2^24 | 2^24 + 1 keys", lambda c: c["name"] == "ks-2^24", dict(form=DR.SMALL, passes=3), lambda c: c["name"] == "ks-2^24+1", dict(form=DR.SMALL, passes=4)),
    ("2^32 | more keys through the tables", lambda c: c["name"] == "ks-2^32-two-tables", dict(form=DR.SMALL, passes=4),
     lambda c: c["name"] == "ks-3x2^31", dict(form=DR.LARGE, passes=5)),
    ("2^32 | more rows in one table", lambda c: c["name"] == "ks-2^32-one-table", dict(form=DR.SMALL, passes=4),
     lambda c: c["name"] == "ks-64bit-100", dict(form=DR.LARGE, passes=5)),
    ("the 64-bit sort: 4 | 5 passes", lambda c: c["name"] == "large-4-passes", dict(form=DR.LARGE, passes=4), lambda c: c["name"] == "ks-64bit-100", dict(form=DR.LARGE, passes=5)),
    ("the 64-bit sort: 1 | 8 passes", lambda c: c["name"] == "n-16385", dict(form=DR.LARGE, passes=1), lambda c: c["name"] == "large-8-passes", dict(form=DR.LARGE, passes=8)),
    ("one | several tables: never tstart for one", lambda c: c["name"] == "n-65", dict(tstart=0), lambda c: c["name"] == "tstart-7", dict(tstart=1)),
    ("S = 256 | 4097 slice ids", lambda c: c["name"] == "S-256", dict(tstart=0), lambda c: c["name"] == "S-4097", dict(tstart=1)),
    ("S = 4096 | 4097 slice ids", lambda c: c["name"] == "S-4096", dict(tstart=0), lambda c: c["name"] == "S-4097", dict(tstart=1)),
    ("96 | 97 work-groups of the wide plan", lambda c: c["name"] == "S-257-few-rows", dict(tstart=0), lambda c: c["name"] == "S-257-many-rows", dict(tstart=1)),
    ("kDedupMaxTables | + 1 tables", lambda c: c["name"] == "tables-1023", dict(tstart=1), lambda c: c["name"] == "tables-1024", dict(tstart=0)),
    ("dd_scan_kernel: one | two trips", lambda c: c["name"] == "scan-1048576" and DR.scan_trips(c["N"]) == 1, dict(form=DR.LARGE, nblk=1024, passes=3),
     lambda c: c["name"] == "scan-1048577" and DR.scan_trips(c["N"]) == 2, dict(form=DR.LARGE, nblk=1025, passes=3)),
]


def make_stream(c, stream):
    """-> (indices [N], tableidx [N]); the lookups in no particular order (the map does not need table-major bags)"""
    rs = np.random.RandomState(zlib.crc32(f"{c['name']}/{stream}".encode()) & 0x7FFFFFFF)
    tables, N = c["tables"], c["N"]
    E = DR.rows_of(c["p"])
    allk = tables * E
    if stream == "uniform":      # a pool of about N / 3 keys: duplicates whatever the key space
        pool = rs.randint(0, allk, size=max(1, N // 3), dtype=np.int64)
        keys = pool[rs.randint(0, pool.size, size=N)]
    elif stream == "same":       # one pair -- the LARGEST key: every bit the key space has
        keys = np.full(N, allk - 1, dtype=np.int64)
    elif stream == "distinct":
        assert allk >= N
        keys = rs.permutation(allk)[:N].astype(np.int64)
    elif stream == "ends":       # only the smallest and the largest key of every table
        keys = rs.randint(0, tables, size=N).astype(np.int64) * E + np.where(rs.rand(N) < 0.5, 0, E - 1)
    elif stream == "empty_tables":   # the first, a middle and the last table without a lookup
        live = np.setdiff1d(np.arange(tables), [0, tables // 2, tables - 1])
        keys = live[rs.randint(0, live.size, size=N)].astype(np.int64) * E + rs.randint(0, E, size=N, dtype=np.int64)
    elif stream == "few":
        keys = rs.randint(0, allk, size=5, dtype=np.int64)[rs.randint(0, 5, size=N)]
    elif stream == "heads":      # uniform over the whole key space: nearly all distinct, a run head in every block of 1024
        keys = rs.randint(0, allk, size=N, dtype=np.int64)
    else:
        assert stream == "clamp"
        pool = rs.randint(0, allk, size=max(1, N // 3), dtype=np.int64)
        keys = pool[rs.randint(0, pool.size, size=N)]
    idx, tb = keys % E, keys // E
    if stream == "clamp" and N >= 40:   # duplicates that are equal only AFTER the clamp: the last row five ways, row 0 three ways
        at = rs.choice(N, 20, replace=False)
        idx[at[:10]] = [E - 1, E, E + 5, E - 1, E + (1 << 40), -1, 0, -(1 << 40), 0, -7]
        tb[at[:5]] = tables - 1
        tb[at[5:10]] = 0
        if tables > 1:                  # ... and tables beyond either end
            tb[at[10:20]] = [-1, 0, -5, tables, tables - 1, tables + 7, -1, tables, 0, tables - 1]
            idx[at[10:20]] = 3 % E
    return idx.astype(np.int64), tb.astype(np.int64)


# ---- the library side ----------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


_REPORT = []


def note(what, **figures):
    """a measured figure: printed, and kept for profiles/dedup_tolerances.md (TTX_DEDUP_REPORT=<file>: JSON lines)"""
    print(f"[dedup-routes] {what}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))
    path = os.environ.get("TTX_DEDUP_REPORT")
    if path:
        if not _REPORT:
            import atexit
            atexit.register(lambda: open(path, "a").writelines(json.dumps(r) + "\n" for r in _REPORT))
        _REPORT.append(dict(what=what, **figures))


def build_map(E, c, ti, ttab, fill):
    """ttx_dedup_build of the case through the TEST library, the dd buffer pre-filled with `fill` -> (dd bytes on the host, route)"""
    import ctypes as C

    g = E._geom(c["tables"], c["p"], Q3, R3)
    N, d = c["N"], dev()
    with E.test_library() as L:
        db, nb = L.ttx_dedup_bytes(C.byref(g), N), L.ttx_plan_bytes(C.byref(g), N)
        assert db > 0, "the library does not map this batch"
        dd = torch.full((db,), fill, dtype=torch.uint8, device=d)
        buf = torch.empty(nb, dtype=torch.uint8, device=d)
        E.debug_dd_route(clear=True)
        E._check(L.ttx_dedup_build(C.byref(g), N, ti.data_ptr(), ttab.data_ptr(), dd.data_ptr(), db, buf.data_ptr(), nb, E._stream(d)))
        route = E.debug_dd_route()
    torch.cuda.synchronize()
    return dd.cpu().numpy(), route


def map_regions(lay, exp, N, tables, tstart):
    """(name, byte offset, dtype, count) of what a build must have written"""
    nu = exp["nu"]
    out = [("nu", lay["nu"][0], np.int32, 1)]
    out += [(k, lay[k][0], lay[k][1], n) for k, n in (("uidx", nu), ("utab", nu), ("iota", N), ("uid", N), ("occ", N), ("occ_off", nu + 1))]
    if tstart:
        out.append(("tstart", lay["tstart"][0], np.int64, tables + 1))
    return out


MAP_PARAMS = [(c, s) for c in MAP_CASES for s in c["streams"]]


@pytest.mark.parametrize("c,stream", MAP_PARAMS, ids=[f"{c['name']}-{s}" for c, s in MAP_PARAMS])
def test_map_arrays_and_route(c, stream):
    import tt_embeddings as E

    what = f"{c['name']}/{stream}"
    tables, N = c["tables"], c["N"]
    idx, tb = make_stream(c, stream)
    exp = DR.expected_map(tables, c["p"], idx, tb)
    lay = DR.carve(N)
    want = _rt(c)
    ti, ttab = t(idx), t(tb)
    bufs = []
    for fill in (0x00, 0xA5):
        dd, route = build_map(E, c, ti, ttab, fill)
        got = {k: route[k] for k in ("form", "bpw", "passes", "nblk", "tstart")}
        print(f"[dedup-routes] {what}: N {N} tables {tables} nu {exp['nu']} route {got}")
        assert got == {k: want[k] for k in got}, f"{what}: the library chose {got}, dedup_ref.route says {want}"
        assert dd.size >= lay["map_bytes"]
        for name, o, dt, n in map_regions(lay, exp, N, tables, want["tstart"]):
            arr = np.frombuffer(dd[o:o + n * np.dtype(dt).itemsize].tobytes(), dtype=dt)
            ref = np.asarray([exp["nu"]] if name == "nu" else exp[name][:n])
            assert np.array_equal(arr, ref), (f"{what}: {name} differs from the stable sort by key at "
                                              f"{np.flatnonzero(arr != ref)[:5].tolist()} (fill {fill:#x})")
        if not want["tstart"]:
            o = lay["tstart"][0]
            assert (dd[o:o + 8 * (tables + 1 if tables <= DR.DEDUP_MAX_TABLES else DR.DEDUP_MAX_TABLES + 1)] == fill).all(), \
                f"{what}: tstart was written although the plan of the pairs does not group its tables"
        bufs.append(dd)
    for name, o, dt, n in map_regions(lay, exp, N, tables, want["tstart"]):
        nb = n * np.dtype(dt).itemsize
        assert np.array_equal(bufs[0][o:o + nb], bufs[1][o:o + nb]), f"{what}: two builds differ in {name}"


# ---- (b) the sums, end to end ------------------------------------------------------------------------------------------------------
# run layouts: counts per pair in key order (positions of the sorted occurrence list; a slice = 32 positions)
LAYOUTS = {
    # [0,5) [5,32): inside a slice, the second ENDS on position 31; [32,64): exactly a slice from position 0; [64,74): from position 0;
    # [74,104): a short crossing run; [104,256): crosses, covers the slices 4, 5, 6 whole and ENDS on the last position of slice 7;
    # seven single lookups; [263,333): crosses two boundaries, ends inside; four singles -> 337 positions (no multiple of 32)
    "edges": [5, 27, 32, 10, 30, 152] + [1] * 7 + [70] + [1] * 4,
    "tiny": [3, 1, 9, 1, 6],            # N = 20 < 32: one partial slice
    # [0,2048): 64 slices from a slice start (the LAST one-group fold); [2048,4097): 65 slices (cooperative); 30 singles;
    # [4127,6177): 2050 from position 31 of a slice = 66 slices (cooperative), ends in slice 193; 28 singles; [6205,6215): a short
    # crossing run that ends in slice 194 -- the same work-group of 16 slices (192..207) as the cooperative one; 2 singles
    "long": [2048, 2049] + [1] * 30 + [2050] + [1] * 28 + [10] + [1] * 2,
}
GEOM = {   # D -> (p, q, padded ranks)
    12: (P3, Q3, R3), 16: (P3, [2, 4, 2], R3), 72: (P3, [3, 4, 6], R3), 128: (P3, [4, 8, 4], R3), 18: (P3, [2, 3, 3], R3),
    15: ([14, 15], [3, 5], [1, 4, 1]), 64: ([20, 22, 25], [4, 4, 4], [1, 16, 16, 1]),
}


def ecase(name, D, layout=None, bags=None, span=None, tables=1, psw=False, misaligned=False, B=12):
    p, q, r = GEOM[D]
    return dict(name=name, D=D, p=p, q=q, r=r, layout=layout, bags=bags, span=span, tables=tables, psw=psw, misaligned=misaligned, B=B)


E2E_CASES = []
for _l in LAYOUTS:
    E2E_CASES += [ecase(f"{_l}-D{_d}", _d, layout=_l) for _d in (16, 72, 128, 15, 18)]
    E2E_CASES += [ecase(f"{_l}-D16-misaligned", 16, layout=_l, misaligned=True), ecase(f"{_l}-D16-weights", 16, layout=_l, psw=True),
                  ecase(f"{_l}-D16-three-tables", 16, layout=_l, tables=3)]
E2E_CASES += [ecase("edges-D64-specialised", 64, layout="edges"), ecase("long-D64-specialised-weights", 64, layout="long", psw=True),
              ecase("long-D18-weights", 18, layout="long", psw=True)]
# pool_gather_kernel: leading and trailing empty bags, lengths 0 1 15 16 17 32 33, the last bag ends at N
POOL_BAGS = [0, 0, 1, 15, 16, 17, 0, 32, 33, 0, 0]
E2E_CASES += [ecase("pool-D16", 16, bags="pool"), ecase("pool-D18", 18, bags="pool"), ecase("pool-D16-weights", 16, bags="pool", psw=True),
              ecase("pool-D15-weights", 15, bags="pool", psw=True)]
# pool_gather4_kernel | pool_gather_kernel<float4> on either side of kPoolSpanMin
E2E_CASES += [ecase("span-65537", 16, span=65537), ecase("span-65536", 16, span=65536), ecase("span-65537-weights", 16, span=65537, psw=True)]


def span_bags(N, rs):
    """bag lengths of a batch of N lookups for the wave-span pooling (a span = 64 consecutive lookups): span 0 = 64 one-lookup bags;
    a bag from lane 0 of span 1 running 200 lookups (span 2 has NO head); bags of 5 and 50; a bag from lane 63 of span 4 running 81
    lookups on (82 in all); then ragged bags with empty ones between; the last bag ends at N"""
    lens = [1] * 64 + [200, 5, 50, 82]
    assert sum(lens[:64]) == 64 and sum(lens[:67]) % 64 == 63
    left = N - sum(lens)
    while left > 0:
        n = int(min(left, rs.randint(0, 41)))
        lens.append(n)
        left -= n
    return lens + [0, 0]


def make_e2e(c):
    """-> dict(indices, offsets, rowidx, tableidx, B, N, psw or None, counts or None)"""
    rs = np.random.RandomState(zlib.crc32(c["name"].encode()) & 0x7FFFFFFF)
    tables, p = c["tables"], c["p"]
    E = DR.rows_of(p)
    counts = None
    if c["layout"]:
        counts = LAYOUTS[c["layout"]]
        ui, ut = DR.pairs_from_counts(tables, p, counts, seed=5)
        idx, tb = np.repeat(ui, counts), np.repeat(ut, counts)
        order = np.lexsort((rs.rand(idx.size), tb))        # table-major, the lookups of a table shuffled
        idx, tb = idx[order], tb[order]
        B = c["B"]
        lens = []
        for k in range(tables):
            w = rs.rand(B) * (rs.rand(B) > 0.2)
            w[rs.randint(B)] += 1e-3
            lens.append(rs.multinomial(int((tb == k).sum()), w / w.sum()))
        lens = np.concatenate(lens)
    else:
        lens = np.array(POOL_BAGS if c["bags"] else span_bags(c["span"], rs), dtype=np.int64)
        B = lens.size
        pool = rs.permutation(E)[:max(8, min(E, int(lens.sum()) // 3))]
        idx = pool[rs.randint(0, pool.size, size=int(lens.sum()))].astype(np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rowidx, tableidx = R.rowidx_from_offsets(off, tables)
    N = int(off[-1])
    psw = (rs.rand(N) * 1.5 + 0.25).astype(np.float32) if c["psw"] else None
    return dict(indices=idx.astype(np.int64), offsets=off, rowidx=rowidx, tableidx=tableidx, B=int(B), N=N, psw=psw, counts=counts)


def e2e_route(c, N):
    return DR.route(c["tables"], c["p"], N, c["D"], aligned=not c["misaligned"], pool_aligned=True)


def run_shared(E, c, b, cores, state0, d_out):
    """forward, dense gradients, fused SGD and fused Adagrad of the case on ONE map, through the test library
    -> dict(out, grads, sgd, ada_w, ada_s, route)"""
    tables, p, q, r, D, B, N = c["tables"], c["p"], c["q"], c["r"], c["D"], b["B"], b["N"]
    T = len(p)
    ti, trow, ttab = t(b["indices"]), t(b["rowidx"]), t(b["tableidx"])
    w = None if b["psw"] is None else t(b["psw"])
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    if c["misaligned"]:   # d_output one float behind a 16-byte address: the pre-sum takes its scalar kernels at D % 4 == 0
        flat = torch.empty(d_out.size + 1, dtype=torch.float32, device=dev())
        dd = flat[1:].view(tables, B, D)
        dd.copy_(t(d_out))
        assert dd.data_ptr() % 16 == 4 and dd.is_contiguous()
    else:
        dd = t(d_out)
        assert dd.data_ptr() % 16 == 0
    args = (p, q, r, Lt, N, ti, trow, ttab, dd)
    with E.test_library():
        E.debug_dd_route(clear=True)
        plan = E.make_plan(tables, p, q, r, N, ti, ttab, trow, dedup=True)
        assert isinstance(plan, E.DedupPlan)
        dc = [t(x) for x in cores]
        out = E.tt_forward(1000, tables, B, D, p, q, r, Lt, N, ti, trow, ttab, dc, plan=plan, per_sample_weights=w).cpu().numpy()
        grads = [x.cpu().numpy() for x in E.tt_dense_backward(1000, D, *args, dc, plan=plan, per_sample_weights=w)]
        E.tt_sgd_backward(1000, D, LR, *args, dc, plan=plan, per_sample_weights=w)
        sgd = [x.cpu().numpy() for x in dc]
        dc, ds = [t(x) for x in cores], [t(x) for x in state0]
        E.tt_adagrad_backward(1000, D, LR, EPS, *args, ds, dc, plan=plan, per_sample_weights=w)
        route = E.debug_dd_route()
    torch.cuda.synchronize()
    dmap = plan.dd.cpu().numpy()
    return dict(out=out, grads=grads, sgd=sgd, ada_w=[x.cpu().numpy() for x in dc], ada_s=[x.cpu().numpy() for x in ds], route=route, dd=dmap)


@pytest.mark.parametrize("c", E2E_CASES, ids=[c["name"] for c in E2E_CASES])
def test_sums_end_to_end(c):
    import tt_embeddings as E

    what = c["name"]
    tables, p, q, r, D = c["tables"], c["p"], c["q"], c["r"], c["D"]
    T = len(p)
    b = make_e2e(c)
    B, N = b["B"], b["N"]
    seed = zlib.crc32(what.encode()) & 0xFFFF
    cores = G.make_cores(seed + 1, tables, p, q, r, "signed")
    d_out = G.make_grad(seed + 2, tables, B, D)
    ref = R.forward_backward(tables, p, q, r, B, b["indices"], b["rowidx"], b["tableidx"], cores, d_out, per_sample_weights=b["psw"])
    state0, _ = R.live_state(ref["grads"], ref["touched"], seed + 3)
    mask = R.slice_mask(ref["touched"], cores)
    got, again = run_shared(E, c, b, cores, state0, d_out), run_shared(E, c, b, cores, state0, d_out)
    # ---- the route and the map this run stood on
    want = e2e_route(c, N)
    assert got["route"] == want, f"{what}: the library chose {got['route']}, dedup_ref.route says {want}"
    exp = DR.expected_map(tables, p, b["indices"], b["tableidx"])
    lay = DR.carve(N)
    for name, o, dt, n in map_regions(lay, exp, N, tables, want["tstart"]):
        arr = np.frombuffer(got["dd"][o:o + n * np.dtype(dt).itemsize].tobytes(), dtype=dt)
        assert np.array_equal(arr, [exp["nu"]] if name == "nu" else exp[name][:n]), f"{what}: {name} of the map"
    if b["counts"] is not None:
        assert np.array_equal(np.diff(exp["occ_off"]), b["counts"]), f"{what}: the runs are not the layout the case names"
    # ---- forward: bit-identical to the plain path, within tolerance of float64
    ti, trow, ttab = t(b["indices"]), t(b["rowidx"]), t(b["tableidx"])
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    plain = E.tt_forward(1000, tables, B, D, p, q, r, Lt, N, ti, trow, ttab, [t(x) for x in cores],
                         plan=E.make_plan(tables, p, q, r, N, ti, ttab, trow), per_sample_weights=None if b["psw"] is None else t(b["psw"])).cpu().numpy()
    assert np.array_equal(got["out"], plain), f"{what}: the forward is not bit-identical to the plain path"
    note(f"{what} out", N=N, units=R.default_units(got["out"], ref["out"]))
    assert_close(got["out"], ref["out"], f"{what} out vs float64")
    # ---- dense gradients, fused SGD, fused Adagrad from a live state
    e_sgd = R.sgd_step(cores, ref["grads"], LR)
    e_w, e_s = R.adagrad_step(cores, state0, ref["grads"], ref["touched"], LR, EPS)
    for k in range(T):
        note(f"{what} core{k}", grad=R.default_units(got["grads"][k], ref["grads"][k]), sgd=R.default_units(got["sgd"][k], e_sgd[k]),
             adagrad_state=R.default_units(got["ada_s"][k], e_s[k]), adagrad_weights=R.default_units(got["ada_w"][k], e_w[k]))
        assert not got["grads"][k][~mask[k]].any(), f"{what} grad{k}: an untouched slice has a gradient"
        assert_close(got["grads"][k], ref["grads"][k], f"{what} grad{k} vs float64")
        assert np.array_equal(got["sgd"][k][~mask[k]], cores[k][~mask[k]]), f"{what} sgd core{k}: an untouched slice changed"
        assert_close(got["sgd"][k], e_sgd[k], f"{what} sgd core{k} vs float64")
        assert np.array_equal(got["ada_w"][k][~mask[k]], cores[k][~mask[k]]) and np.array_equal(got["ada_s"][k][~mask[k]], state0[k][~mask[k]]), \
            f"{what} adagrad core{k}: an untouched slice changed"
        R.assert_state_close(got["ada_s"][k], e_s[k], ref["grads"][k], f"{what} adagrad state{k} vs float64")
        assert_adagrad_close(got["ada_w"][k], e_w[k], ref["grads"][k], f"{what} adagrad core{k} vs float64", lr=LR, eps=EPS, state0=state0[k])
    # ---- a second run: bit-identical
    assert again["route"] == want
    assert np.array_equal(got["out"], again["out"]), f"{what}: out differs between two runs"
    for key in ("grads", "sgd", "ada_w", "ada_s"):
        for k in range(T):
            assert np.array_equal(got[key][k], again[key][k]), f"{what}: {key}[{k}] differs between two runs"
