"""The lookup plan (csrc/ttx_plan.hip) at the sizes that switch its route, ARRAY BY ARRAY against a stable sort in numpy.

Every kernel of a training step reads the plan; plan_build, plan_build_mb and prologue_fusable choose between seven ways of
building it (tiny, single launch -- also as the lookup prologue --, wave units, one wide digit of 10 / 11 / 12 bits, a wide digit
per table group, 8-bit passes, several batches in one launch) and DESIGN 4.1 says they all produce the same, deterministic plan.
Here every case is built THROUGH THE TEST LIBRARY, which reports the route it took (ttx_debug_plan_route) and where carve_plan
put the arrays (ttx_debug_plan_layout); the route must be the one tests/plan_ref.py::route expects, and the arrays must EQUAL
plan_ref.expected -- integer work has one right answer, and an unstable order, which no float comparison sees, fails too.

Cases: both sides of every threshold of the choice (THRESHOLDS below; tests/test_plan_routes_cpu.py holds the table against
plan_ref.route, so that a retuned constant cannot silently take a side away), with the skewed index streams on the "at
capacity" side -- ALL of them on every such case, a partial-wave size beyond a one-pass threshold takes three as well --: uniform; every lookup in one slice of every core; every slice used, round-robin; the first and the last slice id
of every core empty, and then the only ones used; pivot runs of exactly MC, MC + 1, 3 MC and 17 MC + 1 lookups; indices the
decode clamps.  The sizes N + 1 beyond a threshold are no multiples of 64 (1025, 16385, ...): a last partial wave everywhere.

What is compared, per array of the `Plan` comment in csrc/ttx_internal.h (n = the live count):
  hdr            [0] = sum over the pivot's slices of ceil(len / MC), [1] = MC, [2] = n, [3] = 1 with bag rows given and 0 without
                 (the norows-* cases: one per place that writes the word; lrow is then not compared), [20] = 0;
                 [8 + t]: the rule of tests/test_fused_optimizer_gpu.py -- the true number of slices beyond the hot threshold or
                 -1 for a thin core; for the pivot the true number on the routes that count it (finish_single_pass), else -1, or 0
                 when there is none
  perm[t], ipos[t], off[t]   t != 1: on EVERY route, exactly
  lrec, lrow, chunk_off      on EVERY route, exactly (lrec.x is the pivot's sorted order)
  chunk_rec      its invariants (plan_ref.check_chunks: the ORDER of the list is a route's own), and zeros behind hdr[0]
  off[1]         on the routes that write it (table groups, 8-bit passes: mb_chunks_kernel reads it there).  The tiny, single,
                 units and wide routes leave it UNWRITTEN: their finish code writes chunk_off for the pivot, and no consumer reads
                 off[1] -- every read of Plan::off outside ttx_plan.hip is `(t == 1) ? P.chunk_off : sel_core(P.off, t)`
                 (ttx_tt.hip reduce_apply, three places), the `else` of a `t == 1` test (ttx_tt.hip:1115) or P.off[2] / P.off[3]
                 (t4 kernels); search: `(\\.|->)(sid|perm|off|ipos)\\b` over csrc/ outside ttx_plan.hip
  perm[1], ipos[1]           written by NO route (the pivot's order lives in lrec.x); the same search finds reads of ipos[0],
                 ipos[2], ipos[3] only (ttx_tt.hip, ttx_tt_spec.inc, ttx_tt_generic.inc) and none of perm
  sid[t]         written only by the 8-bit passes for a core that needs more than one (later passes chase order -> key); checked
                 there.  Nothing outside ttx_plan.hip reads Plan::sid (the same search: only local variables of that name)
Both builds of a case (into buffers pre-filled with different bytes) must agree on every checked array byte for byte.

End to end, for the cases of at most 70,000 lookups: forward, dense gradients and fused Adagrad from tt_ref64.live_state against
the float64 reference tests/tt_ref64.py at the default tolerance of tests/util.py; a case WITH a hot slice may be wider by the
existing rule only (tt_ref64.widen_factor: twice the fp32 oracle's own distance from float64, capped at 5e-5 / 1e-5).  Left out:
the clamped-index stream (the float64 reference takes in-range indices only) and device-side counts below N.  Above 70,000
lookups only the plan is checked (test_plan_paths_vs_oracle runs those routes through the kernels).

What the end-to-end half found (the plan of both cases was exact): units-65536-one_slice and units-65536-ends_only missed the
dense gradient of core 2 at the CAPPED bound -- 2305.2178 for 2304.8689 (1.5e-4 relative, 7 of 50 elements) and -163.61314 for
-163.59956 (8.3e-5).  Core 2's slice is 10 floats, no multiple of 4, so it stays with reduce_apply_kernel's scalar owner however
hot it is, and that owner added its 65,536 (32,768) same-sign rows into ONE running fp32 sum.  It now sums blocks of 256 rows and
then the block sums (csrc/ttx_tt.hip); the two cases are the regression test."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import gen_inputs as G
import plan_ref as PR
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

Q3, R3 = [2, 3, 2], [1, 4, 5, 1]          # generic and cheap
P3 = [7, 6, 5]
P64 = [1700, 1700, 1700]                  # prod(p) > 2^32: the 64-bit decode
MIXED = [[60, 6, 5], [35, 4, 7]]
MC_NOMINAL = 16                           # lookups per chunk of these geometries (asserted against the library's on the GPU)
E2E_MAX = 70000

FULL = ("uniform", "one_slice", "each_once", "ends_empty", "ends_only", "pivot_runs")
FAR = ("uniform",)
FAR_SKEWED = ("uniform", "one_slice", "ends_only", "pivot_runs")   # a last partial wave under a skewed stream too


def case(name, tables, p, N, streams, entry="build", live=None, B=48, q=Q3, r=R3, nbatch=1, rows=True):
    return dict(name=name, tables=tables, p=p, N=N, streams=streams, entry=entry, live=live, B=B, q=q, r=r, nbatch=nbatch, rows=rows)


CASES = [
    # ---- N = 1024 | 1025: tiny <-> the rest, three ways
    case("tiny-1024", 1, P3, 1024, FULL + ("clamp",)), case("tiny-1025", 1, P3, 1025, FAR + ("clamp",)),
    case("tiny64-1024", 1, P64, 1024, FULL), case("tiny64-1025", 1, P64, 1025, FAR),
    case("tinydev-1024", 1, P3, 1024, FULL, entry="build_n", live=1024),
    # ---- N thresholds of the one-digit routes
    case("single-16384", 1, P3, 16384, FULL), case("single-16385", 1, P3, 16385, FAR_SKEWED),
    case("units-65536", 1, P3, 65536, FULL), case("units-65537", 1, P3, 65537, FAR_SKEWED),
    case("units-1048576", 1, P3, 1 << 20, FULL), case("units-1048577", 1, P3, (1 << 20) + 1, FAR_SKEWED),
    case("wide-393216", 1, [300, 6, 5], 393216, FULL),
    case("wide-393217", 1, [300, 6, 5], 393217, FAR),
]
for _s in (256, 1024, 2048, 4096, 65536):   # ---- S = largest count of slice ids in a core
    CASES += [case(f"S-{_s}", 1, [_s, 6, 5], 3000, FULL), case(f"S-{_s + 1}", 1, [_s + 1, 6, 5], 3000, FAR)]
CASES += [
    case("S-65537-every-slice", 1, [65537, 6, 5], 66000, ("each_once",)),
    # ---- S reached through the table id, mixed tables, other core counts
    case("S-by-table-2", 2, [100, 6, 5], 3000, FULL), case("S-by-table-3", 3, [100, 6, 5], 3000, ("uniform", "one_slice", "ends_only")),
    case("mixed-1000", 2, MIXED, 1000, FULL), case("mixed-3000", 2, MIXED, 3000, ("uniform", "ends_only", "pivot_runs")),
    case("T2-single", 1, [40, 50], 3000, ("uniform", "pivot_runs"), q=[2, 3], r=[1, 4, 1]),
    case("T2-passes", 1, [5000, 6], 3000, ("uniform", "ends_only"), q=[2, 3], r=[1, 4, 1]),
    case("T4-single", 1, [5, 6, 7, 8], 3000, ("uniform", "pivot_runs"), q=[2, 3, 2, 2], r=[1, 4, 5, 3, 1]),
    case("T4-wide", 1, [5, 300, 7, 8], 3000, ("uniform", "ends_only"), q=[2, 3, 2, 2], r=[1, 4, 5, 3, 1]),
    # ---- table groups: ttx_lookup_prologue with table-major offsets
    case("group-span-1024", 5, [1024, 6, 5], 5000, FULL, entry="prologue"),
    case("group-span-1025", 5, [1025, 6, 5], 5000, FAR, entry="prologue"),
    case("group-span-2048", 3, [2048, 6, 5], 5000, FULL, entry="prologue"),
    case("group-span-2049", 3, [2049, 6, 5], 5000, FAR, entry="prologue"),
    case("group-tables-32", 32, [200, 6, 5], 5000, FULL, entry="prologue", B=8),
    case("group-tables-33", 33, [200, 6, 5], 5000, ("uniform", "ends_only"), entry="prologue", B=8),
    case("group-rows-96", 2, [200, 6, 5], 786431, FULL, entry="prologue"),
    case("group-rows-97", 2, [200, 6, 5], 786432, FAR, entry="prologue"),
    # ---- the fused prologue: 4096 | 4097 bags, one table, 1024 < N <= 16384
    case("prologue-4096", 1, P3, 5000, FULL, entry="prologue", B=4096),
    case("prologue-4097", 1, P3, 5000, FAR, entry="prologue", B=4097),
    # ---- several batches in one launch: 16 | 17
    # (the batches of a launch take the streams of FULL in turn: batch z has stream FULL[z % 6])
    case("multi-16", 1, P3, 2000, FULL, entry="multi", B=64, nbatch=16), case("multi-17", 1, P3, 2000, FULL, entry="multi", B=64, nbatch=17),
    # ---- no bag rows (rowidx = NULL): hdr[3] = 0 and lrow unwritten, once per place that writes the word -- the tiny kernel,
    # finish_single_pass (single launch, wave units), finish_wide, mb_chunks_kernel
    case("norows-tiny", 1, P3, 1000, FAR, rows=False), case("norows-single", 1, P3, 3000, FAR, rows=False),
    case("norows-units", 1, P3, 20000, FAR, rows=False), case("norows-wide", 1, [300, 6, 5], 3000, FAR, rows=False),
    case("norows-passes", 1, [4097, 6, 5], 3000, FAR, rows=False),
]
# ---- a device-side count of 0, 1, N - 1, N, with N sizing the buffers on the far side of a threshold
for _tag, _p, _n in (("single", P3, 1025), ("units", P3, 16385), ("wide", [300, 6, 5], 3000), ("passes", [4097, 6, 5], 3000)):
    CASES += [case(f"dev-{_tag}-{_n}-live-{_l}", 1, _p, _n, FAR, entry="build_n", live=_l) for _l in (0, 1, _n - 1, _n)]


class Derived:
    """what the choice of a route looks at, for one case"""

    def __init__(self, c, mc=MC_NOMINAL):
        self.c, self.name, self.N, self.entry, self.nbatch = c, c["name"], c["N"], c["entry"], c["nbatch"]
        self.g = g = PR.Geom(c["tables"], c["p"])
        self.tables, self.mixed, self.idx32, self.smax = g.tables, g.mixed, g.idx32, max(g.S)
        self.n_dev, self.live = c["live"] is not None, c["live"]
        self.nb = c["tables"] * c["B"]
        self.gsz, self.ngroups, self.span, self.grows = PR.group_shape(g, self.N)
        self.route = PR.route(g, self.N, mc, n_dev=self.n_dev, entry=self.entry, nb=self.nb)


def _plain(d):
    return d.entry == "build" and not d.n_dev and not d.mixed and d.tables == 1 and d.g.T == 3 and d.c["rows"]


def _by_s(lo, r_lo, r_hi):
    return (f"S = {lo} | {lo + 1}", lambda d: _plain(d) and d.N == 3000 and d.smax == lo, {r_lo},
            lambda d: _plain(d) and d.N == 3000 and d.smax == lo + 1, {r_hi})


def _grouped(d):
    return d.entry == "prologue" and d.tables > 1


# (label, cases of the near side, the routes they must take, cases of the far side, theirs)
THRESHOLDS = [
    ("N = 1024 | 1025: tiny <-> single", lambda d: _plain(d) and d.idx32 and d.smax <= 256 and d.N == 1024, {PR.TINY},
     lambda d: _plain(d) and d.idx32 and d.smax <= 256 and d.N == 1025, {PR.SINGLE}),
    ("N = 1024 | 1025 with prod(p) > 2^32: never tiny", lambda d: not d.idx32 and not d.mixed and d.N == 1024, {PR.WIDE11},
     lambda d: not d.idx32 and not d.mixed and d.N == 1025, {PR.WIDE11}),
    ("N = 1024 | 1025 with a device-side count: never tiny", lambda d: d.n_dev and d.live == d.N == 1024, {PR.SINGLE},
     lambda d: d.n_dev and d.live == d.N == 1025, {PR.SINGLE}),
    ("N = 16384 | 16385: single <-> units", lambda d: _plain(d) and d.N == 16384, {PR.SINGLE}, lambda d: _plain(d) and d.N == 16385, {PR.UNITS}),
    ("N = 65536 | 65537: the unit grows", lambda d: _plain(d) and d.N == 65536 and PR.unit_positions(d.N) == 256, {PR.UNITS},
     lambda d: _plain(d) and d.N == 65537 and PR.unit_positions(d.N) == 320, {PR.UNITS}),
    ("N = 1048576 | + 1: units <-> passes", lambda d: _plain(d) and d.N == 1 << 20, {PR.UNITS},
     lambda d: _plain(d) and d.N == (1 << 20) + 1, {PR.MULTIPASS + 1}),
    ("N = 393216 | 393217 with 256 < S <= 4096: wide <-> passes", lambda d: _plain(d) and 256 < d.smax <= 4096 and d.N == 393216, {PR.WIDE10},
     lambda d: _plain(d) and 256 < d.smax <= 4096 and d.N == 393217, {PR.MULTIPASS + 2}),
    _by_s(256, PR.SINGLE, PR.WIDE10), _by_s(1024, PR.WIDE10, PR.WIDE11), _by_s(2048, PR.WIDE11, PR.WIDE12),
    _by_s(4096, PR.WIDE12, PR.MULTIPASS + 2), _by_s(65536, PR.MULTIPASS + 2, PR.MULTIPASS + 3),
    ("S through the table id", lambda d: d.entry == "build" and d.tables == 2 and not d.mixed and d.smax == 200, {PR.SINGLE},
     lambda d: d.entry == "build" and d.tables == 3 and d.smax == 300, {PR.WIDE10}),
    ("mixed tables leave the single launch at any N", lambda d: d.mixed and d.N <= 1024 and d.smax <= 256, {PR.WIDE10},
     lambda d: d.mixed and 1024 < d.N <= 16384 and d.smax <= 256, {PR.WIDE10}),
    ("group size x p_max = 1024 | 1025", lambda d: _grouped(d) and d.span == 1024, {PR.GROUPED10}, lambda d: _grouped(d) and d.span == 1025, {PR.GROUPED11}),
    ("group size x p_max = 2048 | 2049", lambda d: _grouped(d) and d.span == 2048, {PR.GROUPED11}, lambda d: _grouped(d) and d.span == 2049, {PR.MULTIPASS + 2}),
    ("32 | 33 tables: one <-> two tables per group", lambda d: _grouped(d) and d.tables == 32 and d.gsz == 1, {PR.GROUPED10},
     lambda d: _grouped(d) and d.tables == 33 and d.gsz == 2, {PR.GROUPED10}),
    ("96 | 97 count rows per group", lambda d: _grouped(d) and d.grows == 96, {PR.GROUPED10}, lambda d: _grouped(d) and d.grows == 97, {PR.MULTIPASS + 2}),
    ("the fused prologue: 4096 | 4097 bags", lambda d: d.entry == "prologue" and d.tables == 1 and d.nb == 4096, {PR.SINGLE_PROLOGUE},
     lambda d: d.entry == "prologue" and d.tables == 1 and d.nb == 4097, {PR.SINGLE}),
    ("16 | 17 batches in one launch", lambda d: d.entry == "multi" and d.nbatch == 16, {PR.MULTIBATCH}, lambda d: d.entry == "multi" and d.nbatch == 17, {PR.MULTIBATCH}),
]


# ---- index streams -------------------------------------------------------------------------------------------------------------
def make_batch(c, stream, mc, salt=0):
    """-> (indices [N], offsets [tables * B + 1]): table-major ragged bags, a fifth of them empty; the lookups of a table shuffled"""
    rs = np.random.RandomState(zlib.crc32(f"{c['name']}/{stream}/{salt}".encode()) & 0x7FFFFFFF)
    g = PR.Geom(c["tables"], c["p"])
    N, B, T = c["N"], c["B"], g.T
    share = rs.rand(g.tables) + 0.5
    if stream == "one_slice" and g.tables > 2:
        share[1] = 0.0                                                   # an empty table (an empty group still writes its offsets)
    n_k = rs.multinomial(N, share / share.sum())
    idx_all, lens_all = [], []
    for k in range(g.tables):
        n, pk = int(n_k[k]), [int(x) for x in g.p_tables[k]]
        idx = np.zeros(n, dtype=np.int64)
        for t in range(T):
            p = pk[t]
            if stream == "one_slice":
                col = np.full(n, (p - 1) // 2, dtype=np.int64)
            elif stream == "each_once":
                col = rs.permutation(p)[np.arange(n) % p]
            elif stream == "ends_empty" and p >= 3:
                col = rs.randint(1, p - 1, size=n)
            elif stream == "ends_only":
                col = np.where(rs.rand(n) < 0.5, 0, p - 1)
            elif stream == "pivot_runs" and t == 1 and p >= 5:
                runs = [r_ for r_ in (mc, mc + 1, 3 * mc, 17 * mc + 1)]
                while sum(runs) > n:
                    runs.pop()
                col = np.concatenate([np.full(r_, dg, dtype=np.int64) for dg, r_ in enumerate(runs)] + [np.zeros(0, dtype=np.int64)])
                col = np.concatenate([col, rs.randint(len(runs), p, size=n - col.size)])
                rs.shuffle(col)
            else:
                col = rs.randint(0, p, size=n)
            idx = idx * p + col.astype(np.int64)
        if stream == "clamp" and n >= 8:
            idx[rs.choice(n, 4, replace=False)] = [-1, -(1 << 40), g.rows[k], g.rows[k] + 12345]
        w = rs.rand(B) * (rs.rand(B) > 0.2)
        w[rs.randint(B)] += 1e-3
        idx_all.append(idx)
        lens_all.append(rs.multinomial(n, w / w.sum()))
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens_all))]).astype(np.int64)
    return np.concatenate(idx_all), off


# ---- the library side ----------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _vp(x):
    return None if x is None else C.c_void_p(x.data_ptr())


def build_plan(E, c, ti, toff, trow, ttab, fill):
    """one plan of the case through the TEST library, into a buffer pre-filled with `fill` -> (buf, route id, rowidx, tableidx)"""
    g = E._geom(c["tables"], c["p"], c["q"], c["r"])
    N, d = c["N"], dev()
    if not c["rows"]:
        assert c["entry"] == "build"
        trow = None
    with E.test_library() as L:
        nb = L.ttx_plan_bytes(C.byref(g), N)
        buf = torch.full((nb,), fill, dtype=torch.uint8, device=d)
        st = C.c_void_p(E._stream(d))
        if c["entry"] == "build":
            E._check(L.ttx_plan_build(C.byref(g), N, _vp(ti), _vp(ttab), _vp(trow), _vp(buf), nb, st))
        elif c["entry"] == "build_n":
            nd = torch.tensor([c["live"]], dtype=torch.int32, device=d)
            E._check(L.ttx_plan_build_n(C.byref(g), N, _vp(nd), _vp(ti), _vp(ttab), _vp(trow), _vp(buf), nb, st))
        else:
            assert c["entry"] == "prologue"
            trow, ttab = torch.full_like(ti, -7), torch.full_like(ti, -7)
            E._check(L.ttx_lookup_prologue(C.byref(g), N, _vp(ti), toff.numel() - 1, _vp(toff), 0, None, None, _vp(trow), _vp(ttab),
                                           _vp(buf), nb, st))
        route = E.debug_plan_route()
    torch.cuda.synchronize()
    return buf, route, trow, ttab


def hot_rule(hdr, exp, route, T, what):
    """hdr[8 + t]: tests/test_fused_optimizer_gpu.py's rule"""
    for k in range(T):
        nh, got = exp["hot"][k], int(hdr[8 + k])
        if k == 1 and route not in PR.ONE_LAUNCH_COUNTS_PIVOT:
            assert got == -1 or (nh == 0 and got == 0), f"{what}: hot pivot slices {got} in the plan, {nh} here"
        else:
            assert got in ((-1, nh) if k != 1 else (nh,)), f"{what}: hot slices of core {k}: {got} in the plan, {nh} here"


def check_plan(lay, buf, exp, route, g, mc, what, rows=True):
    """every array the plan's consumers read, against the reference (the module docstring says which route writes what)
    -> [(offset, length)] of the checked regions, in ints"""
    v = buf.view(torch.int32)
    n, T = exp["n"], g.T
    regions = []

    def arr(key, count=None):
        o, ln = lay[key]
        count = ln if count is None else count
        assert count <= ln
        regions.append((o, count))
        return v[o:o + count].cpu().numpy()

    hdr = arr("hdr", 24)
    assert int(hdr[1]) == mc and int(hdr[2]) == n and int(hdr[3]) == (1 if rows else 0) and int(hdr[20]) == 0, f"{what}: header {hdr[:24]}"
    hot_rule(hdr, exp, route, T, what)
    h0 = lay["hdr"][0]
    regions[-1:] = [(h0, 4), (h0 + 8, T), (h0 + 20, 1)]   # (the header words a build writes: the others keep the buffer's bytes)
    passes = [PR.passes_of(s) for s in g.S]
    multipass = PR.MULTIPASS < route < PR.MULTIBATCH
    grouped = PR.GROUPED10 <= route <= PR.GROUPED11
    for k in range(T):
        if k != 1:
            assert np.array_equal(arr(("perm", k), n), exp["perm"][k]), f"{what}: perm[{k}] is not the stable sort by slice id"
            assert np.array_equal(arr(("ipos", k), n), exp["ipos"][k]), f"{what}: ipos[{k}] is not the inverse of perm[{k}]"
        if k != 1 or multipass or grouped:
            assert np.array_equal(arr(("off", k)), exp["off"][k]), f"{what}: off[{k}]"
        if multipass and passes[k] > 1:
            assert np.array_equal(arr(("sid", k), n), exp["sid"][k]), f"{what}: sid[{k}]"
    lrec = arr("lrec", 4 * n).reshape(n, 4)
    assert np.array_equal(lrec[:, 0], exp["lrec"][:, 0]), f"{what}: the pivot's order (lrec.x) is not the stable sort by its slice id"
    assert np.array_equal(lrec, exp["lrec"]), f"{what}: lrec's slice ids of the other cores"
    if rows:   # (hdr[3] == 0: lrow is not valid, the consumers take the bag rows from their own rowidx argument)
        assert np.array_equal(arr("lrow", n), exp["lrow"]), f"{what}: lrow"
    rec = arr("chunk_rec").reshape(-1, 4)
    assert rec.shape[0] == lay["max_chunks"]
    hdr0 = int(hdr[0])
    assert 0 <= hdr0 <= lay["max_chunks"], f"{what}: hdr[0] = {hdr0} of at most {lay['max_chunks']} chunks"
    try:
        PR.check_chunks(exp, mc, hdr0, rec, arr("chunk_off"))
    except AssertionError as ex:
        raise AssertionError(f"{what}: {ex}") from None
    assert not rec[hdr0:].any(), f"{what}: records behind hdr[0] are not zero"
    return regions


def reference(c, g, idx, off, mc):
    rowidx, tableidx = R.rowidx_from_offsets(off, c["tables"])
    n = c["N"] if c["live"] is None else c["live"]
    return rowidx, tableidx, PR.expected(g, idx[:n], tableidx[:n], rowidx[:n], mc)


PARAMS = [(c, s) for c in CASES if c["entry"] != "multi" for s in c["streams"]]


@pytest.mark.parametrize("c,stream", PARAMS, ids=[f"{c['name']}-{s}" for c, s in PARAMS])
def test_plan_arrays_route_and_results(c, stream):
    import tt_embeddings as E

    what = f"{c['name']}/{stream}"
    g = PR.Geom(c["tables"], c["p"])
    N = c["N"]
    lay = E.debug_plan_layout(c["tables"], c["p"], c["q"], c["r"], N)
    mc = lay["MC"]
    assert mc == MC_NOMINAL and lay["T"] == g.T, f"{what}: the library cuts chunks of {mc} lookups"
    idx, off = make_batch(c, stream, mc)
    assert idx.size == N and off[-1] == N
    rowidx, tableidx, exp = reference(c, g, idx, off, mc)
    ti, toff, trow, ttab = t(idx), t(off), t(rowidx), t(tableidx)
    want = PR.route(g, N, mc, n_dev=c["live"] is not None, entry=c["entry"], nb=c["tables"] * c["B"])
    bufs = []
    for fill in (0x00, 0xA5):
        buf, route, orow, otab = build_plan(E, c, ti, toff, trow, ttab, fill)
        print(f"[plan-routes] {what}: N {N} S {g.S} route {route} ({PR.route_name(route)}), expected {want} ({PR.route_name(want)})")
        assert route == want, f"{what}: the library took route {PR.route_name(route)}, plan_ref.route says {PR.route_name(want)}"
        if c["entry"] == "prologue":
            assert np.array_equal(orow.cpu().numpy(), rowidx) and np.array_equal(otab.cpu().numpy(), tableidx), f"{what}: the prologue's bag rows / tables"
        regions = check_plan(lay, buf, exp, route, g, mc, what, rows=c["rows"])
        bufs.append(buf.view(torch.int32))
    for o, ln in regions:
        assert torch.equal(bufs[0][o:o + ln], bufs[1][o:o + ln]), f"{what}: two builds differ in the ints [{o}, {o + ln}) of the plan"
    if N <= E2E_MAX and stream != "clamp" and c["live"] in (None, N):
        end_to_end(E, c, g, idx, rowidx, tableidx, ti, trow, ttab, E.Plan(buf, N, None), exp, what)


def make_cores(c, g, seed):
    if not g.mixed:
        return G.make_cores(seed, c["tables"], [int(x) for x in g.p_tables[0]], c["q"], c["r"], "signed")
    rs = np.random.RandomState(seed)   # tables of different row factors: one array of all their slices per core
    return [np.ascontiguousarray(rs.uniform(-1.0, 1.0, size=(1, g.S[k], c["r"][k] * c["q"][k] * c["r"][k + 1])) / np.sqrt(max(c["r"][k] * c["r"][k + 1], 1)),
                                 dtype=np.float32) for k in range(g.T)]


def oracle(O, c, g, idx, rowidx, tableidx, cores, d_out):
    """the fp32 oracle's forward and dense gradients of the case -> (out [tables, B, D], [T] gradients of the cores' shapes);
    tables of different row factors one by one (the oracle takes one factoring), their slices side by side as in the cores"""
    tables, q, r, B = c["tables"], c["q"], c["r"], c["B"]
    D = int(np.prod(q))
    if not g.mixed:
        og = O.make_geom(tables, c["p"], q, r)
        return (O.tt_forward(og, B, D, idx, rowidx, tableidx, cores),
                O.tt_backward(og, O.OPTIM_DENSE, B, D, 0, 0, idx, rowidx, tableidx, d_out, [x.copy() for x in cores]))
    outs, grads = [], [[] for _ in range(g.T)]
    for k in range(tables):
        m = tableidx == k
        pk = [int(x) for x in g.p_tables[k]]
        ck = [np.ascontiguousarray(cores[j][:, int(g.base[j][k]):int(g.base[j][k]) + pk[j]]) for j in range(g.T)]
        og = O.make_geom(1, pk, q, r)
        zeros = np.zeros(int(m.sum()), dtype=np.int64)
        outs.append(O.tt_forward(og, B, D, idx[m], rowidx[m], zeros, ck)[0])
        gk = O.tt_backward(og, O.OPTIM_DENSE, B, D, 0, 0, idx[m], rowidx[m], zeros, d_out[k:k + 1], [x.copy() for x in ck])
        for j in range(g.T):
            grads[j].append(gk[j])
    return np.stack(outs), [np.concatenate(x, axis=1) for x in grads]


def end_to_end(E, c, g, idx, rowidx, tableidx, ti, trow, ttab, plan, exp, what):
    """forward, dense gradients, fused Adagrad from a live state on THIS plan against float64"""
    import oracle_lib as O

    tables, p, q, r, B, N, T = c["tables"], c["p"], c["q"], c["r"], c["B"], c["N"], g.T
    D = int(np.prod(q))
    cores = make_cores(c, g, 17 + N)
    d_out = G.make_grad(19 + N, tables, B, D)
    ref = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores, d_out)
    hot = any(exp["hot"])
    f_out, fg = 1.0, [1.0] * T
    if hot:   # the only widening: the fp32 oracle's own distance from float64 on this case
        o_out, o_g = oracle(O, c, g, idx, rowidx, tableidx, cores, d_out)
        f_out, u = R.widen_factor(o_out, ref["out"])
        fg = [R.widen_factor(o_g[k], ref["grads"][k])[0] for k in range(T)]
        print(f"[plan-routes] {what}: hot slices {exp['hot']}; bounds x{f_out:.2f} (out, oracle at {u:.3f}), x{[round(f, 2) for f in fg]} (gradients)")
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    dd = t(d_out)
    dc = [t(x) for x in cores]
    out = E.tt_forward(1000, tables, B, D, p, q, r, Lt, N, ti, trow, ttab, dc, plan=plan).cpu().numpy()
    print(f"[plan-routes] {what} out: {R.default_units(out, ref['out']):.3f} default bounds from float64")
    assert_close(out, ref["out"], f"{what} out vs float64", rtol=RTOL * f_out, atol_scale=ATOL_SCALE * f_out)
    grads = [x.cpu().numpy() for x in E.tt_dense_backward(1000, D, p, q, r, Lt, N, ti, trow, ttab, dd, dc, plan=plan)]
    mask = R.slice_mask(ref["touched"], cores)
    for k in range(T):
        print(f"[plan-routes] {what} grad{k}: {R.default_units(grads[k], ref['grads'][k]):.3f} default bounds from float64")
        assert not grads[k][~mask[k]].any(), f"{what} grad{k}: an untouched slice has a gradient"
        assert_close(grads[k], ref["grads"][k], f"{what} grad{k} vs float64", rtol=RTOL * fg[k], atol_scale=ATOL_SCALE * fg[k])
    state0, _ = R.live_state(ref["grads"], ref["touched"], 23 + N)
    e_w, e_s = R.adagrad_step(cores, state0, ref["grads"], ref["touched"], LR, EPS)
    dc, ds = [t(x) for x in cores], [t(x) for x in state0]
    E.tt_adagrad_backward(1000, D, LR, EPS, p, q, r, Lt, N, ti, trow, ttab, dd, ds, dc, plan=plan)
    for k in range(T):
        w, s = dc[k].cpu().numpy(), ds[k].cpu().numpy()
        assert np.array_equal(w[~mask[k]], cores[k][~mask[k]]) and np.array_equal(s[~mask[k]], state0[k][~mask[k]]), \
            f"{what} adagrad core{k}: an untouched slice changed"
        print(f"[plan-routes] {what} adagrad core{k}: state {R.default_units(s, e_s[k]):.3f}, weights {R.default_units(w, e_w[k]):.3f} "
              f"default bounds from float64")
        R.assert_state_close(s, e_s[k], ref["grads"][k], f"{what} adagrad state{k} vs float64", scale=fg[k])
        assert_adagrad_close(w, e_w[k], ref["grads"][k], f"{what} adagrad core{k} vs float64", lr=LR, eps=EPS, state0=state0[k], scale=fg[k])


MULTI = [c for c in CASES if c["entry"] == "multi"]


@pytest.mark.parametrize("c", MULTI, ids=[c["name"] for c in MULTI])
def test_multi_batch_launch_equals_the_plans_built_alone(c):
    """ttx_lookup_prologue_multi: 16 batches are one launch, 17 are two; every batch's plan must be byte-identical, over the checked
    arrays, to the plan ttx_lookup_prologue builds of that batch alone -- and equal to the reference; the last batch end to end"""
    import tt_embeddings as E

    g = PR.Geom(c["tables"], c["p"])
    N, nbatch, d = c["N"], c["nbatch"], dev()
    lay = E.debug_plan_layout(c["tables"], c["p"], c["q"], c["r"], N)
    mc = lay["MC"]
    assert mc == MC_NOMINAL
    one = dict(c, entry="prologue")
    batches = [make_batch(c, c["streams"][z % len(c["streams"])], mc, salt=z) for z in range(nbatch)]
    tis, toffs = [t(b[0]) for b in batches], [t(b[1]) for b in batches]
    gg = E._geom(c["tables"], c["p"], c["q"], c["r"])
    want = PR.route(g, N, mc, entry="multi", nb=c["tables"] * c["B"])
    with E.test_library() as L:
        L.ttx_lookup_prologue_multi.argtypes = [C.POINTER(type(gg)), C.c_int32, C.c_int64, C.POINTER(C.c_void_p), C.c_int64, C.POINTER(C.c_void_p),
                                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        stride = (L.ttx_plan_bytes(C.byref(gg), N) + 255) // 256 * 256
        plans = torch.full((nbatch * stride,), 0x5A, dtype=torch.uint8, device=d)
        rows, tabs = torch.full((nbatch * N,), -7, dtype=torch.int64, device=d), torch.full((nbatch * N,), -7, dtype=torch.int64, device=d)
        E._check(L.ttx_lookup_prologue_multi(C.byref(gg), nbatch, N, E._ptr_array(tis), c["tables"] * c["B"], E._ptr_array(toffs), 0, None, None,
                                             _vp(rows), _vp(tabs), _vp(plans), stride, C.c_void_p(E._stream(d))))
        route = E.debug_plan_route()
    torch.cuda.synchronize()
    print(f"[plan-routes] {c['name']}: route {route} ({PR.route_name(route)}), expected {want} ({PR.route_name(want)})")
    assert route == want == PR.MULTIBATCH
    for z in range(nbatch):
        what = f"{c['name']} batch {z}"
        idx, off = batches[z]
        rowidx, tableidx, exp = reference(one, g, idx, off, mc)
        assert np.array_equal(rows[z * N:(z + 1) * N].cpu().numpy(), rowidx) and not tabs[z * N:(z + 1) * N].any(), f"{what}: bag rows / tables"
        pz = plans[z * stride:(z + 1) * stride]
        regions = check_plan(lay, pz, exp, route, g, mc, what)
        alone, r1, _, _ = build_plan(E, one, tis[z], toffs[z], None, None, 0x00)
        assert r1 == PR.SINGLE_PROLOGUE
        a, b = pz.view(torch.int32), alone.view(torch.int32)
        for o, ln in regions:
            assert torch.equal(a[o:o + ln], b[o:o + ln]), f"{what}: the ints [{o}, {o + ln}) differ from the plan built alone"
    z = nbatch - 1
    idx, off = batches[z]
    rowidx, tableidx, exp = reference(one, g, idx, off, mc)
    end_to_end(E, c, g, idx, rowidx, tableidx, tis[z], t(rowidx), t(tableidx), E.Plan(plans[z * stride:(z + 1) * stride], N, None), exp,
               f"{c['name']} batch {z}")
