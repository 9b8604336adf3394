"""The fused backward (ttx_tt_backward: gradient + SGD / Adagrad in reduce_apply_kernel and t4_apply23_kernel) against the float64
reference tests/tt_ref64.py, ONE CASE PER APPLY SITE, Adagrad from a LIVE state.

The optimizer update is written out at seven places (csrc/ttx_tt.hip): ApplyEmit in the wave-per-slice packed owner, in the hot
pivot slices' column work-groups, in the last-arriver fold of the thin cores' segment work-groups and in the float4 slice owner;
on their own the scalar slice owner (slice sizes that are not multiples of 4), t4_apply23_kernel (the merged last cores of a
four-core shape) and -- through the float4 owner's code -- the owner fall-back when more than kMaxHotPivot pivot slices are hot.
Which one a slice takes depends on the batch.  Every case here is BUILT for one site from the host-side classifier
(tt_ref64.classify_apply_sites, whose thresholds tests/test_tt_ref64_cpu.py pins to the sources) with the chunk length the library
reports, asserts from the classifier that the site is reached, and cross-checks the classifier with the plan the library built
(chunk total, hot-slice counts of the plan header).

Per case: forward, dense gradients, fused SGD, fused Adagrad -- all against float64.  Adagrad starts from tt_ref64.live_state
(every element distinct, half of a slice dominated by the prior state, half by the gradient, one touched slice per core at zero):
a kernel that wrote g^2 instead of s0 + g^2, read another lane's or slice's state, or dropped the read on one site fails.  Beyond
closeness: slices the batch does not touch keep weights and state bit for bit (dense: exactly zero gradient), the dense call leaves
the cores alone, a second run from the same inputs is bit-identical.

Tolerances.  Default (rtol 1e-5, atol 2e-6 max|ref|) for the forward, the dense gradient and the SGD cores.  A comparison is wider
only when the fp32 oracle (oracle/ttx_oracle.c), on the same case, is ITSELF more than half a default bound from float64: then
twice the oracle's distance (an fp32 sum in another order has an independent rounding error of the same size), capped at the
(5e-5, 1e-5) the suite uses for hot slices elsewhere.  The Adagrad state is bounded by that gradient bound carried through s0 + g^2
(tt_ref64.assert_state_close), the weights by util.assert_adagrad_close(state0=, scale=).  Every figure is printed (pytest -s)."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

CAP = 5.0  # (5e-5, 1e-5) in units of the default bound


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- batches with a prescribed number of lookups per slice -------------------------------------------------------------------------
def build_batch(seed, tables, p, B, fixed, bg, n_bg):
    """fixed[k][t] = {digit: lookups} of table k, core t (exactly that many); the table's other lookups -- up to n_bg[k] beyond
    its longest `fixed` column -- fall uniformly on the digits bg[t] (digits in neither stay UNTOUCHED).  The cores' digit columns
    are shuffled independently; bags are ragged, a fifth of them empty.  -> (indices, offsets)"""
    rs = np.random.RandomState(seed)
    T = len(p)
    idx_all, lens_all = [], []
    for k in range(tables):
        fx = fixed.get(k, {})
        n = max([sum(fx.get(c, {}).values()) for c in range(T)] + [0]) + n_bg[k]
        idx = np.zeros(n, dtype=np.int64)
        for c in range(T):
            col = np.concatenate([np.full(cnt, dg, dtype=np.int64) for dg, cnt in fx.get(c, {}).items()] + [np.zeros(0, dtype=np.int64)])
            rest = n - col.size
            free = [dg for dg in bg[c] if dg not in fx.get(c, {})]
            assert rest == 0 or free, f"table {k} core {c}: {rest} lookups and no digit to put them on"
            if rest:
                col = np.concatenate([col, np.asarray(free, dtype=np.int64)[rs.randint(0, len(free), size=rest)]])
            assert (col < p[c]).all()
            rs.shuffle(col)
            idx = idx * p[c] + col
        w = rs.rand(B) * (rs.rand(B) > 0.2)
        w[0] += 1e-3
        idx_all.append(idx)
        lens_all.append(rs.multinomial(n, w / w.sum()))
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens_all))]).astype(np.int64)
    return np.concatenate(idx_all), off


def _exp(cls, core, site, n=None, at_least=1):
    got = cls["cores"][core][site]
    assert (got == n) if n is not None else (got >= at_least), f"core {core}: {got} slices at site {site}; {cls['cores'][core]}"


Q444, R32, R16 = [4, 4, 4], [32, 32], [16, 16]


def _packed_t3(mc):
    fixed = {0: {0: {7: 600, 8: 700, 9: 5}, 1: {3: 16 * mc + 1, 4: 16 * mc}, 2: {11: 513, 12: 512}}}
    bg = [range(0, 200), range(0, 200), range(0, 200)]

    def check(cls):
        assert cls["pack"]
        _exp(cls, 0, "thin_fold", 2), _exp(cls, 0, "packed"), _exp(cls, 2, "thin_fold", 1), _exp(cls, 1, "pivot_columns", 1)
        _exp(cls, 1, "packed"), _exp(cls, 2, "packed")
        assert cls["shared_segments"][0] == 1 and not cls["hot"][2][12] and cls["rows"][1][4] == 16
    return dict(tables=1, p=[400, 500, 450], q=Q444, r=[4, 4], B=200, fixed=fixed, bg=bg, n_bg=[4000], check=check, spec=False)


def _packed_t2(mc):
    fixed = {0: {0: {5: 520, 6: 600}, 1: {9: 16 * mc, 10: 16 * mc + 1}}}

    def check(cls):
        assert cls["pack"]
        _exp(cls, 0, "thin_fold", 2), _exp(cls, 0, "packed"), _exp(cls, 1, "pivot_columns", 1), _exp(cls, 1, "packed")
    return dict(tables=1, p=[600, 700], q=[8, 8], r=[32], B=150, fixed=fixed, bg=[range(300), range(300)], n_bg=[3000], check=check, spec=True)


def _float4_owner(mc):
    def check(cls):
        for c in range(3):
            _exp(cls, c, "float4_owner")
            assert sum(cls["cores"][c].values()) == cls["cores"][c]["float4_owner"] and not cls["hot"][c].any()
    return dict(tables=3, p=[6, 5, 7], q=Q444, r=R32, B=40, fixed={}, bg=[range(5), range(4), range(6)], n_bg=[300, 250, 7], check=check,
                pairs=[(LR, EPS), (0.02, 1e-2)], spec=True)


def _scalar_owner(mc):
    fixed = {0: {0: {1: 600}, 2: {2: 700}}}

    def check(cls):
        for c in range(3):
            _exp(cls, c, "scalar_owner")
            assert sum(cls["cores"][c].values()) == cls["cores"][c]["scalar_owner"]
        assert cls["lens"][0][1] == 600 > 2 * R.SEG_THIN and cls["lens"][2][2] == 700  # (odd hot slices stay with their owner)
    return dict(tables=1, p=[5, 6, 7], q=[3, 3, 5], r=[13, 11], B=60, fixed=fixed, bg=[[0, 2, 3], range(5), [0, 1, 3, 4, 5]], n_bg=[500],
                check=check, spec=True)


def _scalar_padded(mc):
    fixed = {1: {2: {4: 513}}}

    def check(cls):
        _exp(cls, 0, "scalar_owner"), _exp(cls, 1, "float4_owner"), _exp(cls, 2, "thin_fold", 1), _exp(cls, 2, "float4_owner")
    return dict(tables=3, p=[7, 9, 11], q=[3, 4, 5], r=[13, 12], B=50, fixed=fixed, bg=[range(6), range(8), range(10)], n_bg=[400, 300, 350],
                check=check, spec=True)


def _pivot_columns(nh):
    def make(mc):
        hot = {h: 16 * mc + 1 + 7 * h for h in range(nh)}
        fixed = {0: {1: {**hot, 39: 16 * mc}}}

        def check(cls):
            _exp(cls, 1, "pivot_columns", nh), _exp(cls, 1, "pivot_owner_fallback", 0), _exp(cls, 1, "float4_owner")
            assert cls["rows"][1][0] == 17 and cls["rows"][1][39] == 16 and not cls["hot"][1][39]
        return dict(tables=1, p=[3, 40, 3], q=Q444, r=R32, B=80, fixed=fixed, bg=[[0, 1], range(10, 36), [0, 1]], n_bg=[600], check=check,
                    spec=True)
    return make


def _pivot_fallback(nh):
    def make(mc):
        fixed = {0: {1: {h: 16 * mc + 1 + h for h in range(nh)}}}

        def check(cls):
            assert cls["pivot_count_known"], "the owner fall-back needs a plan that COUNTS the hot pivot slices"
            _exp(cls, 1, "pivot_owner_fallback", nh), _exp(cls, 1, "pivot_columns", 0)
        return dict(tables=1, p=[3, 40 if nh < 12 else 12, 3], q=Q444, r=R32, B=80, fixed=fixed, bg=[[0, 1], range(10, 36) if nh < 12 else [], [0, 1]],
                    n_bg=[300 if nh < 12 else 0], check=check, spec=True,
                    all_touched=(1,) if nh == 12 else ())
    return make


def _thin_hot(mc):
    fixed = {1: {0: {0: 100, 1: 600, 2: 700, 3: 512, 4: 513}, 2: {5: 1100, 6: 513}}}

    def check(cls):
        _exp(cls, 0, "thin_fold", 3), _exp(cls, 2, "thin_fold", 2), _exp(cls, 0, "float4_owner"), _exp(cls, 2, "float4_owner")
        assert cls["shared_segments"][0] >= 1, "two hot slices are meant to meet in one segment"
        assert cls["lens"][0][8 + 3] == 2 * R.SEG_THIN and not cls["hot"][0][8 + 3] and cls["hot"][0][8 + 4]
        off = np.concatenate([[0], np.cumsum(cls["lens"][0])])
        # (any hot slice spans segments; this one begins and ends INSIDE one, so both its end segments are shared with neighbours)
        assert off[8 + 1] % R.SEG_THIN != 0 and off[8 + 2] % R.SEG_THIN != 0, "a hot slice is meant to begin and end inside a segment"
    return dict(tables=3, p=[8, 40, 8], q=Q444, r=R16, B=70, fixed=fixed, bg=[[5, 6], range(36), [0, 1, 2]], n_bg=[200, 200, 150], check=check,
                spec=True)


def _t4(q, ranks, tables, mfma):
    def make(mc):
        fixed = {0: {0: {1: 600}, 1: {2: 16 * mc + 1}}}
        r2q2, r3 = ranks[1] * q[2], ranks[2]
        # (the gradient helper of the merged last cores, csrc/ttx_tt.hip ttx_tt_backward: MFMA when its tiles are whole)
        assert (r2q2 % 16 == 0 and r3 % 16 == 0 and r2q2 * r3 // 256 <= 32) == mfma

        def check(cls):
            _exp(cls, 2, "t4_apply23"), _exp(cls, 3, "t4_apply23"), _exp(cls, 1, "pivot_columns", 1)
            _exp(cls, 0, "thin_fold" if (q[0] * ranks[0]) % 4 == 0 else "scalar_owner")
        return dict(tables=tables, p=[5, 40, 4, 5], q=q, r=ranks, B=60, fixed=fixed, bg=[[0, 2, 3], range(4, 36), range(3), range(4)],
                    n_bg=[400] + [150] * (tables - 1), check=check, merged=True, spec=True)
    return make


def _two_cores(mc):
    fixed = {0: {0: {3: 700}, 1: {2: 16 * mc + 1, 3: 16 * mc}}}

    def check(cls):
        assert not cls["pack"]
        _exp(cls, 0, "thin_fold", 1), _exp(cls, 0, "float4_owner"), _exp(cls, 1, "pivot_columns", 1), _exp(cls, 1, "float4_owner")
    return dict(tables=1, p=[9, 40], q=[8, 8], r=[32], B=90, fixed=fixed, bg=[[0, 1, 2, 4, 5, 6, 7], range(4, 36)], n_bg=[600], check=check,
                spec=True)


def _generic(mc):
    fixed = {0: {1: {1: 16 * mc + 1, 2: 16 * mc}, 2: {3: 600}}}

    def check(cls):
        _exp(cls, 1, "pivot_columns", 1), _exp(cls, 2, "thin_fold", 1), _exp(cls, 0, "float4_owner"), _exp(cls, 1, "float4_owner")
    return dict(tables=1, p=[6, 40, 7], q=[5, 3, 4], r=[8, 12], B=60, fixed=fixed, bg=[range(5), range(4, 36), range(6)], n_bg=[500], check=check,
                spec=False)


def _generic_chunk2(mc):
    fixed = {0: {1: {1: 33, 2: 32}}}

    def check(cls):
        _exp(cls, 1, "pivot_columns", 1), _exp(cls, 1, "float4_owner")
        assert cls["rows"][1][1] == 17 and cls["rows"][1][2] == 16 and not cls["pivot_count_known"]
    return dict(tables=1, p=[6, 8, 7], q=[5, 3, 4], r=[8, 12], B=30, fixed=fixed, bg=[range(5), [0, 3, 4], range(6)], n_bg=[60], check=check,
                spec=False, chunk=2)


CASES = {
    "packed_three_cores": _packed_t3,
    "packed_two_cores": _packed_t2,
    "float4_owner_not_hot": _float4_owner,
    "scalar_owner_odd_slices": _scalar_owner,
    "scalar_owner_padded_ranks": _scalar_padded,
    "pivot_columns_1_hot": _pivot_columns(1),
    "pivot_columns_2_hot": _pivot_columns(2),
    "pivot_columns_8_hot": _pivot_columns(8),
    "pivot_owner_fallback_9_hot": _pivot_fallback(9),
    "pivot_owner_fallback_all_12_hot": _pivot_fallback(12),
    "thin_cores_hot_segments": _thin_hot,
    "four_cores_mfma_helper": _t4([2, 4, 4, 2], [32, 32, 32], 1, True),
    "four_cores_valu_helper": _t4([3, 4, 2, 3], [13, 12, 7], 3, False),
    "two_cores": _two_cores,
    "generic_kernels": _generic,
    "generic_kernels_chunk_of_2": _generic_chunk2,
}
CHUNK_KNOB = {"generic_kernels_chunk_of_2": 2}  # (test build only: a hot pivot slice with few lookups; every other case at the library's own settings)


def _header(plan):
    torch.cuda.synchronize()
    return plan.buf[:256].view(torch.int32).cpu().numpy()


def _factor(oracle, ref):
    """how much wider than the default this comparison may be: 1, or twice the oracle's own distance from float64 when that is
    more than half a default bound; capped"""
    u = R.default_units(oracle, ref)
    f = 1.0 if u <= 0.5 else min(2.0 * u, CAP)
    return f, u


def _report(what, got, ref, u_oracle, f):
    print(f"[fused-optimizer] {what}: kernel {R.default_units(got, ref):.3f}, oracle {u_oracle:.3f} default bounds from float64 -> bound x{f:.2f}")


@pytest.mark.parametrize("name", list(CASES))
def test_apply_site_against_float64(name):
    import tt_embeddings as E

    knob = CHUNK_KNOB.get(name, 0)
    if knob:
        E.set_chunk(knob)
    try:
        _run(E, name, knob)
    finally:
        if knob:
            E.set_chunk(0)


def _run(E, name, knob):
    make = CASES[name]
    probe = make(32)
    tables, p, q = probe["tables"], probe["p"], probe["q"]
    T = len(p)
    r = G.pad_ranks(probe["r"], T)
    D, B = int(np.prod(q)), probe["B"]
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    # the library's chunk length for this geometry (below 131,072 lookups it does not depend on the batch): the plan header's
    z = torch.zeros(2000, dtype=torch.int64, device=dev())
    mc = int(_header(E.make_plan(tables, p, q, r, 2000, z, z, z))[1])
    tiles = E.debug_tiles(tables, p, q, r)
    # (every case names its kernel family: the specialised kernels report no chunk length of their own)
    assert (tiles["MC"] == 0) == probe["spec"], f"{name}: kernel family, {tiles}"
    if tiles["MC"]:
        assert tiles["MC"] == mc, f"{name}: ttx_debug_tiles reports {tiles['MC']} lookups per chunk, the plan {mc}"
    assert (E.lib().ttx_debug_state() == 0) == (knob == 0), "a case without a knob runs at the library's own settings"
    spec = make(mc)
    merged = bool(spec.get("merged"))
    idx, off = build_batch(sum(map(ord, name)), tables, p, B, spec["fixed"], spec["bg"], spec["n_bg"])
    nnz = idx.size
    assert nnz < 131072
    rowidx, tableidx = R.rowidx_from_offsets(off, tables)
    cls = R.classify_apply_sites(idx, tableidx, tables, p, q, r, mc, merged_last_cores=merged)
    print(f"[fused-optimizer] {name}: nnz {nnz} mc {mc} pack {cls['pack']} sites {cls['cores']}")
    spec["check"](cls)  # the site this case is named for is reached

    cores = G.make_cores(17 + nnz, tables, p, q, r, "signed")
    d_out = G.make_grad(19 + nnz, tables, B, D)
    ti = t(idx)
    _, ri, tb, ntt, _ = E.preprocess_indices_sync(ti, t(off), tables, True, e0, e1)
    assert ntt == nnz and np.array_equal(ri.cpu().numpy(), rowidx) and np.array_equal(tb.cpu().numpy(), tableidx)
    plan = E.make_plan(tables, p, q, r, nnz, ti, tb, ri)
    hdr = _header(plan)
    # the classifier against the plan the library built: chunk total, chunk length, hot slices per core
    assert hdr[1] == mc and hdr[2] == nnz and hdr[0] == int(cls["rows"][1].sum()), f"{name}: plan header {hdr[:12]}"
    for c in ([0, 1] if merged else range(T)):
        nh = int(cls["over"][c].sum())
        if c == 1 and not cls["pivot_count_known"]:
            assert hdr[8 + 1] == -1 or (nh == 0 and hdr[8 + 1] == 0), f"{name}: hot pivot slices {hdr[8 + 1]} in the plan, {nh} here"
        else:
            assert hdr[8 + c] in ((-1, nh) if c != 1 else (nh,)), f"{name}: hot slices of core {c}: {hdr[8 + c]} in the plan, {nh} here"
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    dd = t(d_out)
    args = (p, q, r, Lt, nnz, ti, ri, tb, dd)

    # ---- float64 reference and the fp32 oracle's own distance from it ----
    ref = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores, d_out)
    mask = R.slice_mask(ref["touched"], cores)
    for c in range(T):
        assert np.array_equal(ref["touched"][c], cls["lens"][c] > 0)
    g = O.make_geom(tables, p, q, r)
    o_out = O.tt_forward(g, B, D, idx, rowidx, tableidx, cores)
    o_g = O.tt_backward(g, O.OPTIM_DENSE, B, D, 0, 0, idx, rowidx, tableidx, d_out, [x.copy() for x in cores])

    # ---- forward ----
    dc = [t(x) for x in cores]
    out = E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, ti, ri, tb, dc, plan=plan).cpu().numpy()
    f, u = _factor(o_out, ref["out"])
    _report(f"{name} out", out, ref["out"], u, f)
    assert_close(out, ref["out"], f"{name} out vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

    # ---- dense ----
    runs = []
    for rep in range(2):
        dc = [t(x) for x in cores]
        grads = E.tt_dense_backward(1000, D, *args, dc, plan=plan)
        runs.append([x.cpu().numpy() for x in grads])
        for c in range(T):
            assert np.array_equal(dc[c].cpu().numpy(), cores[c]), f"{name}: the dense backward changed core {c}"
    fg = []
    for c in range(T):
        f, u = _factor(o_g[c], ref["grads"][c])
        fg.append(f)
        _report(f"{name} grad{c}", runs[0][c], ref["grads"][c], u, f)
        assert np.array_equal(runs[0][c], runs[1][c]), f"{name} grad{c}: two runs differ"
        assert not runs[0][c][~mask[c]].any(), f"{name} grad{c}: an untouched slice has a gradient"
        assert mask[c].any() and ((~mask[c]).any() or c in spec.get("all_touched", ())), f"{name}: core {c} has no untouched slice"
        assert_close(runs[0][c], ref["grads"][c], f"{name} grad{c} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

    for lr, eps in spec.get("pairs", [(LR, EPS)]):
        # ---- fused SGD ----
        o_w = [x.copy() for x in cores]
        O.tt_backward(g, O.OPTIM_SGD, B, D, lr, 0, idx, rowidx, tableidx, d_out, o_w)
        e_w = R.sgd_step(cores, ref["grads"], lr)
        runs = []
        for rep in range(2):
            dc = [t(x) for x in cores]
            E.tt_sgd_backward(1000, D, lr, *args, dc, plan=plan)
            runs.append([x.cpu().numpy() for x in dc])
        for c in range(T):
            f, u = _factor(o_w[c], e_w[c])
            _report(f"{name} sgd core{c} lr={lr}", runs[0][c], e_w[c], u, f)
            assert np.array_equal(runs[0][c], runs[1][c]), f"{name} sgd core{c}: two runs differ"
            assert np.array_equal(runs[0][c][~mask[c]], cores[c][~mask[c]]), f"{name} sgd core{c}: an untouched slice changed"
            assert_close(runs[0][c], e_w[c], f"{name} sgd core{c} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

        # ---- fused Adagrad from a live state ----
        state0, zeroed = R.live_state(ref["grads"], ref["touched"], 23 + nnz)
        e_w, e_s = R.adagrad_step(cores, state0, ref["grads"], ref["touched"], lr, eps)
        runs = []
        for rep in range(2):
            dc, ds = [t(x) for x in cores], [t(x) for x in state0]
            E.tt_adagrad_backward(1000, D, lr, eps, *args, ds, dc, plan=plan)
            runs.append(([x.cpu().numpy() for x in dc], [x.cpu().numpy() for x in ds]))
        for c in range(T):
            (w, s), (w2, s2) = (runs[0][0][c], runs[0][1][c]), (runs[1][0][c], runs[1][1][c])
            assert ref["touched"][c][zeroed[c]], "one TOUCHED slice per core starts from a zero state"
            assert np.array_equal(w, w2) and np.array_equal(s, s2), f"{name} adagrad core{c}: two runs differ"
            assert np.array_equal(w[~mask[c]], cores[c][~mask[c]]), f"{name} adagrad core{c}: an untouched slice's weights changed"
            assert np.array_equal(s[~mask[c]], state0[c][~mask[c]]), f"{name} adagrad core{c}: an untouched slice's state changed"
            print(f"[fused-optimizer] {name} adagrad core{c} lr={lr} eps={eps}: state {R.default_units(s, e_s[c]):.3f}, "
                  f"weights {R.default_units(w, e_w[c]):.3f} default bounds from float64 (gradient bound x{fg[c]:.2f})")
            R.assert_state_close(s, e_s[c], ref["grads"][c], f"{name} adagrad state{c} vs float64", scale=fg[c])
            assert_adagrad_close(w, e_w[c], ref["grads"][c], f"{name} adagrad core{c} vs float64", lr=lr, eps=eps, state0=state0[c],
                                 scale=fg[c])
