"""per_sample_weights (nn.EmbeddingBag's, mode="sum") against the float64 reference tests/tt_ref64.py, ONE CASE PER WEIGHT SITE.

The library multiplies by a lookup's weight at about twenty places, and which one a lookup takes depends on the geometry and the
batch.  Forward pooling (csrc/ttx_tt.hip): pool_kernel (D % 4 != 0), pool4_kernel (more than kPoolSpanMin lookups),
pool4_small_kernel, F.psw inside spec_fwd_kernel<.., FUSE> (csrc/ttx_tt_spec.inc: offsets and counters given, a specialised
unpadded shape, D % 4 == 0) and the two pool_gather kernels of the dedup route.  Backward of the cores, where the weight scales a
lookup's share of its bag's gradient row: the four gradient-load statements of the specialised backward (per-pass pointers of the
Shape3::GPP shapes, the padded shapes' guarded weight, the single-sub-chunk kernels' unconditional loads, the guarded sub-chunk
walk), the generic kernels' three loads of the bag gradients (csrc/ttx_tt_generic.inc: bwd_load_dx0 at T == 2, float4 / scalar by D % 4), the two-core kernel, and
gsum_slice_kernel<float4 | float> in front of the dedup route's backward.  The weights' own gradient: ttx_tt_forward_wr keeps the
rows and psw_grad_kernel computes d_psw[n] = <d_out[bag(n)], row_n> -- reached through the module's native node only.

Dropping the weights on ONE of these is the failure the unweighted tests cannot see.  Every case here names the site it is built
for and asserts it is reached before comparing anything: the kernel family from ttx_debug_tiles, chunk length and lookup count
from the plan header, the pooling route from the dispatch restated on the host (tt_ref64.pool_route, pinned to the sources by
tests/test_tt_ref64_cpu.py) AND from the number of pooling launches the library's own profile counters see (none when the
contraction kernel pooled), the padded / exact template from ttx_tt_forward_arrive_ints.

Weights (make_weights): one float32 per lookup in [-0.5, 1.5), a tenth exactly 0, permuted independently of the indices; the last
lookup of the batch and of every table away from 1; one bag holds one index three times with three different weights (a kernel
that takes the weight by distinct pair or by bag fails); one bag holds one index twice with weights that sum to zero.

Per case, all against float64: the forward (with and without the bags' offsets), the dense gradients, fused SGD, fused Adagrad
from tt_ref64.live_state; untouched slices bit-identical, the dense call leaves the cores alone, two runs bit-identical.

Tolerances: the default (rtol 1e-5, atol 2e-6 max|ref|); wider only by the rule of tests/test_fused_optimizer_gpu.py -- when the
fp32 oracle, on the one-bag-per-lookup restatement of the same case (tt_ref64.per_lookup_restatement: the oracle's C has no
weights), is itself more than half a default bound from float64: twice that distance, capped at (5e-5, 1e-5).  Every figure is
printed (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

import gen_inputs as G
import tt_ref64 as R
from test_fused_optimizer_gpu import _header, build_batch
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

PROF_POOL = 4  # TTX_PROF_POOL (include/ttx.h): the pooling launches


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- batches and weights -----------------------------------------------------------------------------------------------------------
def _move_to_bag(seg, start, value, count):
    """the table's lookups `seg` with `count` occurrences of `value` moved to positions start .. start + count - 1 (a permutation:
    every slice keeps its number of lookups)"""
    pos = np.flatnonzero(seg == value)[:count]
    assert pos.size == count
    rest = np.delete(seg, pos)
    return np.concatenate([rest[:start], np.full(count, value, dtype=seg.dtype), rest[start:]])


def make_weights(seed, idx, off, tables, B):
    """-> (indices, weights): the indices of table 0 permuted so that one bag starts with one index three times and another with
    one index twice; the weights of the module docstring"""
    rs = np.random.RandomState(seed)
    idx = idx.copy()
    nnz = idx.size
    lens = np.diff(off)
    w = (rs.rand(nnz) * 2.0 - 0.5).astype(np.float32)
    w[rs.rand(nnz) < 0.1] = 0.0
    w = w[rs.permutation(nnz)]
    last = [int(off[(k + 1) * B]) - 1 for k in range(tables) if off[(k + 1) * B] > off[k * B]]
    # two bags of table 0, neither holding the table's last lookup
    n0 = int(off[B])
    seg = idx[:n0].copy()
    vals, cnt = np.unique(seg, return_counts=True)
    assert (cnt >= 3).sum() >= 2, "the batch repeats too few indices"
    v3, v2 = vals[np.argsort(-cnt, kind="stable")[:2]]
    ok = [b for b in range(B) if off[b + 1] < n0]
    a = next(b for b in ok if lens[b] >= 3)
    c = next(b for b in reversed(ok) if lens[b] >= 2 and b != a)
    seg = _move_to_bag(seg, int(off[a]), v3, 3)
    assert c > a
    rest = seg[int(off[a]) + 3:]
    seg = np.concatenate([seg[:int(off[a]) + 3], _move_to_bag(rest, int(off[c]) - int(off[a]) - 3, v2, 2)])
    assert np.array_equal(np.sort(seg), np.sort(idx[:n0]))
    idx[:n0] = seg
    sa, sc = int(off[a]), int(off[c])
    assert idx[sa] == idx[sa + 1] == idx[sa + 2] == v3 and idx[sc] == idx[sc + 1] == v2
    w[sa:sa + 3] = [0.25, 1.375, -0.4375]
    w[sc], w[sc + 1] = 0.46875, -0.46875
    for n, e in enumerate(last):
        w[e] = (-0.375, 1.4375, 0.3125)[n % 3]
    assert abs(float((w == 0).mean()) - 0.1) < 0.06 or nnz < 100
    assert w.min() >= -0.5 and w.max() < 1.5 and all(abs(w[e] - 1.0) > 0.25 and w[e] != 0 for e in last)
    order = np.argsort(idx, kind="stable")
    assert (np.diff(w[order]) < 0).any() and (np.diff(w[order]) > 0).any() and (np.diff(w) < 0).any(), "weights sorted like the indices"
    return idx, w


def _ragged(tables, p, B, bg, n_per_table, fixed=None):
    def make(seed, mc):
        return build_batch(seed, tables, p, B, fixed(mc) if fixed else {}, bg, n_per_table)
    return make


def _dedup_batch(p, B, bg, distinct):
    """every index of the batch 3 .. 20 times, the occurrences shuffled over ragged bags"""
    def make(seed, mc):
        rs = np.random.RandomState(seed)
        rows = set()
        while len(rows) < distinct:
            rows.add(tuple(int(rs.choice(list(b))) for b in bg))
        vals = np.array([int(np.ravel_multi_index(x, p)) for x in sorted(rows)], dtype=np.int64)
        idx = np.repeat(vals, rs.randint(3, 21, size=vals.size))
        rs.shuffle(idx)
        wts = rs.rand(B) * (rs.rand(B) > 0.2)
        wts[0] += 1e-3
        lens = rs.multinomial(idx.size, wts / wts.sum())
        return idx, np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return make


Q444, P657 = [4, 4, 4], [6, 5, 7]
BG657 = [range(5), range(4), range(6)]  # (one slice of every core stays untouched)

# family: "spec" (the shape-specialised kernels and the two- / four-core kernels beside them: ttx_debug_tiles reports no chunk
# length) or "generic".  forward: with (True) / without (False) the bags' offsets -- both unless the case says.  exact: the geometry IS a template (fused pooling possible); False: a padded one.  sites: what the case is for.
CASES = {
    "spec_fused_pooling": dict(tables=1, p=P657, q=Q444, r=[16, 16], B=40, batch=_ragged(1, P657, 40, BG657, [300]), family="spec", exact=True,
                               forward=(True,), sites="F.psw in spec_fwd_kernel<FUSE>"),
    "spec_pooling_launch": dict(tables=1, p=P657, q=Q444, r=[16, 16], B=40, batch=_ragged(1, P657, 40, BG657, [300]), family="spec", exact=True,
                                forward=(False,), sites="pool4_small_kernel; UNC gradient loads"),
    "spec_three_tables": dict(tables=3, p=P657, q=Q444, r=[32, 32], B=40, batch=_ragged(3, P657, 40, BG657, [300, 250, 7]), family="spec",
                              exact=True, sites="tableidx with weights; trailing partial groups"),
    "spec_padded_d60": dict(tables=3, p=[7, 9, 11], q=[3, 4, 5], r=[13, 12], B=50,
                            batch=_ragged(3, [7, 9, 11], 50, [range(6), range(8), range(10)], [400, 300, 350]), family="spec", exact=False,
                            sites="PAD ld_guard weight"),
    "spec_padded_d45": dict(tables=3, p=[5, 6, 7], q=[3, 3, 5], r=[13, 11], B=50,
                            batch=_ragged(3, [5, 6, 7], 50, [range(4), range(5), range(6)], [400, 300, 350]), family="spec", exact=False,
                            sites="PAD ld_guard weight; pool_kernel"),
    "spec_gpp_d1024": dict(tables=1, p=P657, q=[4, 16, 16], r=[32, 32], B=24, batch=_ragged(1, P657, 24, BG657, [200]), family="spec", exact=True,
                           gpp=True, sites="L.gsw"),
    "spec_large_batch": dict(tables=1, p=P657, q=Q444, r=[32, 32], B=512, batch=_ragged(1, P657, 512, BG657, [132001]), family="spec", exact=True,
                             large=True, sites="pool4_kernel; sub-chunk walk (guarded loads)"),
    "dedup_large_batch": dict(tables=1, p=P657, q=Q444, r=[32, 32], B=512, batch=_ragged(1, P657, 512, BG657, [132001]), family="spec", exact=True,
                              large=True, dedup=True, data="spec_large_batch", sites="pool_gather4_kernel; gsum_slice_kernel at many slices"),
    "two_cores": dict(tables=1, p=[9, 40], q=[8, 8], r=[32], B=90, batch=_ragged(1, [9, 40], 90, [range(8), range(4, 36)], [700]), family="spec",
                      exact=None, sites="two-core kernel"),
    "four_cores_mfma_helper": dict(tables=1, p=[5, 40, 4, 5], q=[2, 4, 4, 2], r=[32, 32, 32], B=60,
                                   batch=_ragged(1, [5, 40, 4, 5], 60, [[0, 2, 3], range(4, 36), range(3), range(4)], [450]), family="spec",
                                   exact=None, sites="merged last cores with weights"),
    "four_cores_valu_helper": dict(tables=3, p=[5, 40, 4, 5], q=[3, 4, 2, 3], r=[13, 12, 7], B=60,
                                   batch=_ragged(3, [5, 40, 4, 5], 60, [[0, 2, 3], range(4, 36), range(3), range(4)], [400, 150, 150]),
                                   family="spec", exact=None, sites="merged last cores with weights"),
    "generic_float4_tail": dict(tables=1, p=[6, 40, 7], q=[5, 3, 4], r=[8, 12], B=60,
                                batch=_ragged(1, [6, 40, 7], 60, [range(5), range(4, 36), range(6)], [500], fixed=lambda mc: {0: {1: {1: 16 * mc + 1}}}),
                                family="generic", exact=None, hot_pivot=True, generic_site="float4",
                                sites="generic kernels, T >= 3, D % 4 == 0: the float4 load of the bag gradients"),
    "generic_scalar_tail": dict(tables=1, p=[6, 40, 7], q=[5, 3, 5], r=[8, 12], B=60,
                                batch=_ragged(1, [6, 40, 7], 60, [range(5), range(4, 36), range(6)], [500]),
                                family="generic", exact=None, generic_site="scalar",
                                sites="generic kernels, T >= 3, D % 4 != 0: the scalar load of the bag gradients; pool_kernel"),
    "generic_two_cores": dict(tables=1, p=[9, 40], q=[4, 40], r=[8], B=90, batch=_ragged(1, [9, 40], 90, [range(8), range(4, 36)], [700]),
                              family="generic", exact=None, generic_site="dx0",
                              sites="generic kernels, T == 2 (a q1 beyond the two-core kernel's 32): bwd_load_dx0"),
    "first_factor_8": dict(tables=1, p=P657, q=[8, 8, 8], r=[16, 16], B=40, batch=_ragged(1, P657, 40, BG657, [300]), family="generic", exact=None,
                           generic_site="float4",
                           sites="q0 = 8 on the engine's own route: generic kernels, float4 load (the module's choice of that route: MODULE_CASES)"),
    "dedup_float4": dict(tables=1, p=P657, q=Q444, r=[16, 16], B=60, batch=_dedup_batch(P657, 60, BG657, 40), family="spec", exact=True, dedup=True,
                         sites="pool_gather_kernel<float4>; gsum_slice_kernel<float4>"),
    "dedup_float": dict(tables=1, p=[5, 6, 7], q=[3, 3, 5], r=[13, 11], B=60, batch=_dedup_batch([5, 6, 7], 60, [range(4), range(5), range(6)], 40),
                        family="spec", exact=False, dedup=True, sites="pool_gather_kernel<float>; gsum_slice_kernel<float>"),
}


_DATA = {}


def _data(name, mc):
    """batch, weights, cores, bag gradients, the float64 reference and the oracle's results of a case: computed once (the two cases
    on the large batch share theirs; only the latest is kept) and left unchanged"""
    cs = CASES[name]
    key = cs.get("data", name)
    if key not in _DATA:
        _DATA.clear()
        tables, p, q, B = cs["tables"], cs["p"], cs["q"], cs["B"]
        r = G.pad_ranks(cs["r"], len(p))
        D = int(np.prod(q))
        seed = sum(map(ord, key))
        idx, off = cs["batch"](seed, mc)
        idx, w = make_weights(seed + 1, idx, off, tables, B)
        nnz = idx.size
        rowidx, tableidx = R.rowidx_from_offsets(off, tables)
        cores = G.make_cores(17 + nnz, tables, p, q, r, "signed")
        d_out = G.make_grad(19 + nnz, tables, B, D)
        ref = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores, d_out, per_sample_weights=w)
        plain = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores)
        assert R.default_units(plain["out"], ref["out"]) > 100, "the weights are meant to matter"
        d = dict(idx=idx, off=off, w=w, rowidx=rowidx, tableidx=tableidx, cores=cores, d_out=d_out, ref=ref,
                 oracle=R.oracle_on_restatement(tables, p, q, r, B, idx, rowidx, tableidx, w, cores, d_out, LR))
        _DATA[key] = d
    return _DATA[key]


def _report(what, got, ref, u_oracle, f):
    print(f"[per-sample-weights] {what}: kernel {R.default_units(got, ref):.3f}, oracle {u_oracle:.3f} default bounds from float64 -> bound x{f:.2f}")


def _pool_launches(E, fn):
    """fn() under the library's profile counters -> (its result, the pooling launches it made)"""
    E.profile_enable(1 << PROF_POOL)
    try:
        E.profile_reset()
        res = fn()
        n, _ = E.profile_read(PROF_POOL)
    finally:
        E.profile_enable(0)
    return res, n


@pytest.mark.parametrize("name", list(CASES))
def test_weight_site_against_float64(name):
    import tt_embeddings as E

    cs = CASES[name]
    tables, p, q, B = cs["tables"], cs["p"], cs["q"], cs["B"]
    T = len(p)
    r = G.pad_ranks(cs["r"], T)
    D = int(np.prod(q))
    dedup, large = bool(cs.get("dedup")), bool(cs.get("large"))
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    assert E.lib().ttx_debug_state() == 0, "every case runs at the library's own settings"

    # ---- the kernel family, and the library's chunk length for it ----
    tiles = E.debug_tiles(tables, p, q, r)
    assert (tiles["MC"] == 0) == (cs["family"] == "spec"), f"{name}: kernel family, {tiles}"
    z = torch.zeros(2000, dtype=torch.int64, device=dev())
    mc = int(_header(E.make_plan(tables, p, q, r, 2000, z, z, z))[1])
    assert not tiles["MC"] or tiles["MC"] == mc
    data = _data(name, mc)
    idx, off, w, rowidx, tableidx = data["idx"], data["off"], data["w"], data["rowidx"], data["tableidx"]
    nnz = idx.size
    lens = np.diff(off)
    assert (lens == 0).any()
    geom = E._geom(tables, p, q, r)
    small = nnz <= R.POOL_SPAN_MIN
    if cs["exact"] is not None and D % 4 == 0 and small:
        # (the counters of fused pooling are owed to exactly the unpadded specialised shapes)
        assert (int(E.lib().ttx_tt_forward_arrive_ints(C.byref(geom), nnz)) == nnz) == cs["exact"], f"{name}: exact / padded template"
    if cs.get("gpp"):
        assert q[0] == 4 and (r[1] == 64 or D >= 1024) and cs["exact"], "a Shape3::GPP shape"
    assert large == (not small)
    if large:
        assert nnz >= 131072 and R.pool_route(nnz, D, True, True) == "pool4"
    if cs["family"] == "generic":
        # which of the generic backward's three loads of the bag gradients the case takes (csrc/ttx_tt_generic.inc: bwd_load_dx0 at
        # T == 2 -- the two-core kernel, t2_shape in csrc/ttx_tt.hip, does not take the shape --, else float4 / scalar by D % 4)
        t2 = T == 2 and r[1] <= 128 and q[0] <= 32 and q[1] <= 32 and r[1] * q[1] <= 2048
        site = "dx0" if T == 2 else ("float4" if D % 4 == 0 else "scalar")
        assert not t2 and site == cs["generic_site"], f"{name}: generic site {site}"
    if cs.get("hot_pivot"):
        cls = R.classify_apply_sites(idx, tableidx, tables, p, q, r, mc)
        assert cls["cores"][1]["pivot_columns"] == 1, f"{name}: one hot pivot slice, {cls['cores'][1]}"

    ti, to, tw = t(idx), t(off), t(w)
    _, ri, tb, ntt, _ = E.preprocess_indices_sync(ti, to, tables, True, e0, e1)
    assert ntt == nnz and np.array_equal(ri.cpu().numpy(), rowidx) and np.array_equal(tb.cpu().numpy(), tableidx)
    plan = E.make_plan(tables, p, q, r, nnz, ti, tb, ri, dedup=dedup)
    if dedup:
        assert isinstance(plan, E.DedupPlan), f"{name}: the batch did not qualify for the dedup route"
        torch.cuda.synchronize()
        nd = int(plan.dd[:4].view(torch.int32).item())
        cnt = np.unique(tableidx * int(np.prod(p)) + idx, return_counts=True)[1]
        assert nd == cnt.size and cnt.min() >= 3 and (large or cnt.max() <= 20), f"{name}: {nd} distinct pairs in the map, {cnt.size} here"
    else:
        assert not isinstance(plan, E.DedupPlan)
        hdr = _header(plan)
        assert hdr[2] == nnz, f"{name}: plan header {hdr[:12]}"
        if large:
            assert hdr[1] > R.SPEC_MC32, f"{name}: chunks of {hdr[1]} lookups are not walked in sub-chunks"
        else:
            assert hdr[1] == mc
    print(f"[per-sample-weights] {name}: nnz {nnz} mc {mc} sites: {cs['sites']}")
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    cores, d_out = data["cores"], data["d_out"]
    dd = t(d_out)
    args = (p, q, r, Lt, nnz, ti, ri, tb, dd)

    # ---- float64 reference; the fp32 oracle on the one-bag-per-lookup restatement, for its own distance from float64 ----
    ref = data["ref"]
    mask = R.slice_mask(ref["touched"], cores)
    lr, eps = LR, EPS
    o_out, _, o_g, o_w = data["oracle"]

    # ---- forward: without and with the bags' offsets ----
    f, u = R.widen_factor(o_out, ref["out"])
    for with_off in cs.get("forward", (False, True)):
        dc = [t(x) for x in cores]
        if dedup:
            route, want_launches = "dedup", 1
        else:
            route = R.pool_route(nnz, D, with_off, cs["family"] == "spec" and T == 3, padded=cs["exact"] is False)
            want_launches = 0 if route == "fused" else 1
        out, launches = _pool_launches(E, lambda: E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, ti, ri, tb, dc, plan=plan,
                                                               offsets=to if with_off else None, per_sample_weights=tw).cpu().numpy())
        _report(f"{name} out ({route})", out, ref["out"], u, f)
        assert launches == want_launches, f"{name}: {launches} pooling launches on the route restated as {route}"
        assert_close(out, ref["out"], f"{name} out ({route}) vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
        if with_off and route == "fused":
            arr = E._arrive_cache[(0, E._stream(dev()))]
            assert int(arr.abs().sum()) == 0, "arrival counters were not left zeroed"
    if name == "spec_fused_pooling":
        assert route == "fused"
    if name == "spec_pooling_launch":
        assert route == "pool4_small"
    if name == "spec_three_tables":
        assert route == "fused" and R.pool_route(nnz, D, False, True) == "pool4_small"
    if name == "generic_scalar_tail":
        assert route == "pool_scalar"
    if name == "spec_padded_d45":
        assert route == "pool_scalar"
    if name == "spec_padded_d60":
        assert route == "pool4_small"

    # ---- dense ----
    runs = []
    for rep in range(2):
        dc = [t(x) for x in cores]
        grads = E.tt_dense_backward(1000, D, *args, dc, plan=plan, per_sample_weights=tw)
        runs.append([x.cpu().numpy() for x in grads])
        for c in range(T):
            assert np.array_equal(dc[c].cpu().numpy(), cores[c]), f"{name}: the dense backward changed core {c}"
    fg = []
    for c in range(T):
        f, u = R.widen_factor(o_g[c], ref["grads"][c])
        fg.append(f)
        _report(f"{name} grad{c}", runs[0][c], ref["grads"][c], u, f)
        assert np.array_equal(runs[0][c], runs[1][c]), f"{name} grad{c}: two runs differ"
        assert not runs[0][c][~mask[c]].any(), f"{name} grad{c}: an untouched slice has a gradient"
        assert mask[c].any() and (~mask[c]).any(), f"{name}: core {c} has no untouched slice"
        assert_close(runs[0][c], ref["grads"][c], f"{name} grad{c} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

    # ---- fused SGD ----
    e_w = R.sgd_step(cores, ref["grads"], lr)
    runs = []
    for rep in range(2):
        dc = [t(x) for x in cores]
        E.tt_sgd_backward(1000, D, lr, *args, dc, plan=plan, per_sample_weights=tw)
        runs.append([x.cpu().numpy() for x in dc])
    for c in range(T):
        f, u = R.widen_factor(o_w[c], e_w[c])
        _report(f"{name} sgd core{c}", runs[0][c], e_w[c], u, f)
        assert np.array_equal(runs[0][c], runs[1][c]), f"{name} sgd core{c}: two runs differ"
        assert np.array_equal(runs[0][c][~mask[c]], cores[c][~mask[c]]), f"{name} sgd core{c}: an untouched slice changed"
        assert_close(runs[0][c], e_w[c], f"{name} sgd core{c} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

    # ---- fused Adagrad from a live state ----
    state0, zeroed = R.live_state(ref["grads"], ref["touched"], 23 + nnz)
    e_w, e_s = R.adagrad_step(cores, state0, ref["grads"], ref["touched"], lr, eps)
    runs = []
    for rep in range(2):
        dc, ds = [t(x) for x in cores], [t(x) for x in state0]
        E.tt_adagrad_backward(1000, D, lr, eps, *args, ds, dc, plan=plan, per_sample_weights=tw)
        runs.append(([x.cpu().numpy() for x in dc], [x.cpu().numpy() for x in ds]))
    for c in range(T):
        (wc, s), (w2, s2) = (runs[0][0][c], runs[0][1][c]), (runs[1][0][c], runs[1][1][c])
        assert ref["touched"][c][zeroed[c]], "one TOUCHED slice per core starts from a zero state"
        assert np.array_equal(wc, w2) and np.array_equal(s, s2), f"{name} adagrad core{c}: two runs differ"
        assert np.array_equal(wc[~mask[c]], cores[c][~mask[c]]), f"{name} adagrad core{c}: an untouched slice's weights changed"
        assert np.array_equal(s[~mask[c]], state0[c][~mask[c]]), f"{name} adagrad core{c}: an untouched slice's state changed"
        print(f"[per-sample-weights] {name} adagrad core{c}: state {R.default_units(s, e_s[c]):.3f}, weights "
              f"{R.default_units(wc, e_w[c]):.3f} default bounds from float64 (gradient bound x{fg[c]:.2f})")
        R.assert_state_close(s, e_s[c], ref["grads"][c], f"{name} adagrad state{c} vs float64", scale=fg[c])
        assert_adagrad_close(wc, e_w[c], ref["grads"][c], f"{name} adagrad core{c} vs float64", lr=lr, eps=eps, state0=state0[c], scale=fg[c])


# ---- the weights' own gradient, through the module's native node (ttx_tt_forward_wr keeps the rows, psw_grad_kernel) ----------------
MODULE_CASES = {
    "d64": dict(tables=1, p=P657, q=Q444, r=[16, 16], B=40, bg=BG657, n=[301]),
    "d45": dict(tables=1, p=[5, 6, 7], q=[3, 3, 5], r=[13, 11], B=40, bg=[range(4), range(5), range(6)], n=[301]),
    "d1024": dict(tables=1, p=P657, q=[4, 16, 16], r=[32, 32], B=24, bg=BG657, n=[203]),
    "three_tables": dict(tables=3, p=P657, q=Q444, r=[32, 32], B=40, bg=BG657, n=[300, 250, 7]),
    # q0 = 8: unweighted calls of this module go as two part lookups per index (_forward_split0); a weighted call must leave that
    # route (the part lookups carry no weights) and still be right
    "first_factor_8": dict(tables=1, p=P657, q=[8, 8, 8], r=[16, 16], B=40, bg=BG657, n=[301], split0=True),
}


@pytest.mark.parametrize("name", list(MODULE_CASES))
def test_gradient_of_the_weights_through_the_module(name):
    """w.grad = d_psw[n] = <d_out[bag(n)], row_n> of the float64 reference, beside forward and the cores (sparse=False: their dense
    gradients; fused SGD: one step), on the native node; bags with empty ones, a lookup count that is no multiple of 16
    (psw_grad_kernel gives sixteen lanes to a lookup)"""
    import tt_embeddings_ops as ops

    cs = MODULE_CASES[name]
    tables, p, q, B = cs["tables"], cs["p"], cs["q"], cs["B"]
    T = len(p)
    r = G.pad_ranks(cs["r"], T)
    E_, D = int(np.prod(p)), int(np.prod(q))
    assert ops._native_node() is not None, "the weights' gradient is served by the C++ node only"
    seed = sum(map(ord, name)) + 500
    idx, off = build_batch(seed, tables, p, B, {}, cs["bg"], cs["n"])
    idx, w = make_weights(seed + 1, idx, off, tables, B)
    nnz = idx.size
    assert nnz % 16 != 0 and (np.diff(off) == 0).any()
    rowidx, tableidx = R.rowidx_from_offsets(off, tables)
    cores = G.make_cores(17 + nnz, tables, p, q, r, "signed")
    d_out = G.make_grad(19 + nnz, tables, B, D)
    ref = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores, d_out, per_sample_weights=w)
    mask = R.slice_mask(ref["touched"], cores)
    o_out, o_psw, o_g, o_w = R.oracle_on_restatement(tables, p, q, r, B, idx, rowidx, tableidx, w, cores, d_out, LR)
    e_w = R.sgd_step(cores, ref["grads"], LR)

    def check(what, got, want, oracle):
        f, u = R.widen_factor(oracle, want)
        _report(f"module {name} {what}", got, want, u, f)
        assert_close(got, want, f"module {name} {what} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

    for extra in (dict(sparse=False), dict(sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR)):
        m = ops.TableBatchedTTEmbeddingBag(tables, E_, D, cs["r"], p, q, use_cache=False, weight_dist="uniform", device=dev(), **extra)
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, cores):
                dst.copy_(t(src))
        assert (m.__dict__.get("_split0", 0) > 1) == bool(cs.get("split0")), "the module's part-lookup route"
        tw = t(w).clone().requires_grad_(True)
        out = m(t(idx), t(off), per_sample_weights=tw)
        assert tuple(out.shape) == (tables, B, D)
        check("out", out.detach().cpu().numpy(), ref["out"], o_out)
        out.backward(t(d_out))
        assert tw.grad is not None, "per_sample_weights that require a gradient must get one"
        check(f"d_psw ({'dense' if not extra['sparse'] else 'fused sgd'})", tw.grad.cpu().numpy(), ref["d_psw"], o_psw)
        for c in range(T):
            if not extra["sparse"]:
                got = m.tt_cores[c].grad.cpu().numpy()
                assert not got[~mask[c]].any() and np.array_equal(m.tt_cores[c].detach().cpu().numpy(), cores[c])
                check(f"grad{c}", got, ref["grads"][c], o_g[c])
            else:
                got = m.tt_cores[c].detach().cpu().numpy()
                assert np.array_equal(got[~mask[c]], cores[c][~mask[c]]), f"module {name} sgd core{c}: an untouched slice changed"
                check(f"sgd core{c}", got, e_w[c], o_w[c])
