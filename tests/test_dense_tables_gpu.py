"""GPU tests of the dense member tables: the kernels of csrc/ttx_dense.hip against the float64 restatement
tests/dense_ref.py at the smallest shapes that reach every path, `DenseTableBatchedEmbeddingBag` against one nn.EmbeddingBag per
table, and `MixedTTEmbeddingBag(dense_below=)`.

Tolerance: the suite's default (tests/util.py: rtol 1e-5, atol 2e-6 max|ref|).  A comparison is widened only by the rule of
tests/test_fused_optimizer_gpu.py: when a plain fp32 numpy sum in index order of the same case (dense_ref with dtype=float32) is
itself more than half a default bound from float64, twice that distance is allowed, capped at (5e-5, 1e-5)
(tt_ref64.widen_factor).  Every figure is printed (pytest -s).  The updated weights are bounded by the gradient's bound carried
through the update: SGD is linear in G (lr dG); element-wise Adagrad as util.assert_adagrad_close(state0=, scale=) derives it; the
row-wise form by the same derivative with the row's state (rowwise_bound below)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as DR
import tt_ref64 as R64
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ES = [3, 1, 24, 1460]
PADS = [2, None, 5, 0]


def eng():
    import tt_embeddings as E

    return E


def split_len():
    return eng().dense_bags_info(64, 1000)["split"]


def _split_case(L, D):
    """tables [3, 24], B = 37: row 0 of table 0 is looked up exactly L times, its lookups spread over the bags between others"""
    rs = np.random.RandomState(L)
    B, idx, off = 37, [], [0]
    per = [L // B + (1 if b < L % B else 0) for b in range(B)]
    for b in range(B):
        bag = [0] * per[b] + rs.randint(1, 3, size=2).tolist()
        rs.shuffle(bag)
        idx += bag
        off.append(len(idx))
    for b in range(B):
        idx += rs.randint(0, 24, size=int(rs.randint(0, 4))).tolist()
        off.append(len(idx))
    idx = np.asarray(idx, np.int64)
    assert int((idx[:off[B]] == 0).sum()) == L
    return dict(Es=[3, 24], B=B, D=D, idx=idx, off=np.asarray(off, np.int64), pads=None,
                psw=rs.uniform(0.5, 1.5, size=idx.size).astype(np.float32))


def _general(D, B, seed, **kw):
    idx, off, psw = DR.make_batch(seed, ES, B, pad=PADS, **kw)
    return dict(Es=ES, B=B, D=D, idx=idx, off=off, psw=psw, pads=PADS)


@functools.lru_cache(maxsize=None)
def case(name):
    C = split_len()
    if name == "split_scalar":
        c = _split_case(C + 1, 6)
    elif name.startswith("split"):  # split_<k>_<0|1>: a row with exactly k * C + (0 | 1) lookups
        _, k, more = name.split("_")
        c = _split_case(int(k) * C + int(more), 64)
    elif name == "d64":  # the 16-byte path; a bag of 70 slots (more than the rows in flight); table 2 receives no lookup
        c = _general(64, 37, 1, tie_table=3, silent_table=2, long_bag=(3, 5, 70))
    elif name == "d64_b1":
        c = _general(64, 1, 2, tie_table=3, empty=0)
    elif name == "d64_misaligned":  # a weight view one float off a 16-byte boundary: the scalar path at D = 64
        c = dict(_general(64, 5, 3, tie_table=2), misaligned=True)
    elif name == "d6":
        c = _general(6, 37, 4, tie_table=2, long_bag=(2, 7, 70))
    elif name == "d3_b1":
        c = _general(3, 1, 5, tie_table=3, empty=0)
    elif name == "d260":  # rows wider than 256 floats: the column-block walk
        c = _general(260, 5, 6, tie_table=2, long_bag=(3, 2, 70))
    elif name == "nnz0":
        c = dict(Es=ES, B=4, D=64, idx=np.zeros(0, np.int64), off=np.zeros(17, np.int64), psw=np.zeros(0, np.float32), pads=PADS)
    elif name == "all_padding":  # the tables' padding values and the merged batches' sentinel, nothing else
        B = 4
        idx = np.concatenate([np.full(2 * B, 2), np.full(2 * B, -1), np.full(2 * B, 5), np.full(2 * B, 0)]).astype(np.int64)
        c = dict(Es=ES, B=B, D=64, idx=idx, off=np.arange(0, 8 * B + 1, 2, dtype=np.int64), pads=PADS,
                 psw=np.ones(idx.size, np.float32))
    else:
        raise KeyError(name)
    c = dict(c)
    c["base"] = np.concatenate([[0], np.cumsum(c["Es"])]).astype(np.int64)
    R = int(c["base"][-1])
    rs = np.random.RandomState(77)
    c["w"] = rs.uniform(-1, 1, size=(R, c["D"])).astype(np.float32)
    c["d_out"] = rs.standard_normal((len(c["off"]) - 1, c["D"])).astype(np.float32)
    # a live, all-distinct Adagrad state
    c["s_elem"] = (0.5 + 1e-4 * np.arange(R * c["D"])).reshape(R, c["D"]).astype(np.float32)
    c["s_row"] = (0.5 + 1e-3 * np.arange(R)).astype(np.float32)
    assert np.unique(c["s_elem"]).size == c["s_elem"].size and np.unique(c["s_row"]).size == R
    return c


CASES = ["d64", "d64_b1", "d64_misaligned", "d6", "d3_b1", "d260", "split_1_0", "split_1_1", "split_2_0", "split_2_1",
         "split_scalar", "nnz0", "all_padding"]


@functools.lru_cache(maxsize=None)
def reference(name, mode):
    """float64 and plain-fp32 results of (case, mode), computed once and shared"""
    c = case(name)
    psw = c["psw"] if mode == "sum" else None
    a = (c["w"], c["idx"], c["off"], c["base"], c["B"])
    out, live, arg = DR.forward(*a, mode, c["pads"], psw)
    out32, _, _ = DR.forward(*a, mode, c["pads"], psw, dtype=np.float32)
    G, touched, d_psw = DR.row_grads(*a, c["d_out"], mode, c["pads"], psw)
    G32, _, d_psw32 = DR.row_grads(*a, c["d_out"], mode, c["pads"], psw, dtype=np.float32)
    return dict(out=out, live=live, arg=arg, out32=out32, G=G, touched=touched, d_psw=d_psw, G32=G32, d_psw32=d_psw32, psw=psw)


def dev_weight(c):
    """the case's weights on the device: 16-byte aligned, or -- misaligned -- a contiguous view one float off"""
    R, D = c["w"].shape
    if c.get("misaligned"):
        buf = torch.zeros(R * D + 1, device=DEV)
        w = buf[1:].view(R, D)
        assert w.data_ptr() % 16 == 4 and w.is_contiguous()
    else:
        w = torch.empty((R, D), device=DEV)
        assert w.data_ptr() % 16 == 0
    w.copy_(torch.from_numpy(c["w"]))
    return w


def batch(c, mode):
    psw = torch.from_numpy(c["psw"]).to(DEV) if mode == "sum" else None
    return torch.from_numpy(c["idx"]).to(DEV), torch.from_numpy(c["off"]).to(DEV), psw


def report(what, got, ref, u, f):
    print(f"[dense-tables] {what}: kernel {R64.default_units(got, ref):.3f}, plain fp32 {u:.3f} default bounds from float64 "
          f"-> bound x{f:.2f}")


def grad_bound(G, f):
    g = np.abs(G)
    return f * (ATOL_SCALE * max(float(g.max()) if g.size else 0.0, 1e-30) + RTOL * g)


def own_bound(w):
    return RTOL * np.abs(w) + 2e-7 * max(float(np.abs(w).max()) if w.size else 0.0, 1e-30)


def assert_within(got, ref, tol, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(err).all(), what
    if (err > tol).any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int((err > tol).sum())}/{err.size} out of tolerance; worst at {i}: got {got[i]!r} ref {ref[i]!r} "
                             f"tol {tol[i]:.3e}")


def rowwise_bound(w_ref, s_ref, G, f, lr, eps):
    """w = w0 - lr G / (sqrt(s) + eps), s = s0 + mean_e G_e^2, with G within dG: |dw| <= lr dG / den + lr |G| ds / (2 sqrt(s) den^2),
    ds <= mean_e(2 |G_e| dG_e + dG_e^2) plus two fp32 ulps of s; and the fp32 rounding of w itself"""
    dG = grad_bound(G, f)
    ds = (2 * np.abs(G) * dG + dG * dG).mean(axis=1) + 2 * np.spacing(s_ref.astype(np.float32)).astype(np.float64)
    den = np.sqrt(s_ref) + eps
    dw = lr * dG / den[:, None] + lr * np.abs(G) * (ds / (2 * np.sqrt(s_ref) * den * den))[:, None]
    return own_bound(w_ref) + dw, ds


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("name", CASES)
def test_kernels_against_float64(name, mode):
    E = eng()
    c, ref = case(name), reference(name, mode)
    idx, off, psw = batch(c, mode)
    base, pads = c["base"].tolist(), c["pads"]
    w0 = dev_weight(c)
    d_out = torch.from_numpy(c["d_out"]).to(DEV)
    touched = ref["touched"]
    # ---- forward
    out, live, arg = E.dense_bags_forward(idx, off, base, w0, mode, pads, psw)
    got = out.cpu().numpy()
    if mode == "max":
        assert np.array_equal(got, ref["out"].astype(np.float32)), "max: the output is a selection -- exact"
        assert np.array_equal(arg.cpu().numpy(), ref["arg"]), "max: argmax"
    else:
        f, u = R64.widen_factor(ref["out32"], ref["out"])
        report(f"{name} {mode} forward", got, ref["out"], u, f)
        assert_close(got, ref["out"], f"{name} {mode} forward", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    if mode == "mean":
        assert np.array_equal(live.cpu().numpy(), ref["live"])
    empty = ref["live"] == 0
    assert not got[empty].any(), "a bag without a live slot is exact zeros"
    out2, live2, arg2 = E.dense_bags_forward(idx, off, base, w0, mode, pads, psw)
    assert torch.equal(out, out2) and (arg is None or torch.equal(arg, arg2)), "forward: bit-identical from run to run"
    # ---- the dense gradient
    f, u = R64.widen_factor(ref["G32"], ref["G"])

    def run(optim, state=None, want=False):
        w = dev_weight(c)
        s = None if state is None else torch.from_numpy(state).to(DEV)
        d_w, d_psw = E.dense_bags_backward(optim, idx, off, base, w, d_out, mode, pads, psw, live, arg, LR, EPS, s, want)
        return w, s, d_w, d_psw

    _, _, d_w, d_psw = run(E.OPTIM_DENSE, want=mode == "sum")
    gw = d_w.cpu().numpy()
    report(f"{name} {mode} G", gw, ref["G"], u, f)
    assert_close(gw, ref["G"], f"{name} {mode} dense gradient", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    assert not gw[~touched].any(), "dense: rows the batch does not touch are exactly zero"
    assert torch.equal(d_w, run(E.OPTIM_DENSE)[2]), "dense gradient: bit-identical from run to run"
    # ---- fused SGD, and the weights' gradient from the pre-update weights
    w, _, _, d_psw_f = run(E.OPTIM_SGD, want=mode == "sum")
    gw = w.cpu().numpy()
    want_w = DR.sgd(c["w"], ref["G"], touched, LR)
    assert_within(gw, want_w, own_bound(want_w) + LR * grad_bound(ref["G"], f), f"{name} {mode} sgd weights")
    assert np.array_equal(gw[~touched], c["w"][~touched]), "sgd: untouched rows keep their weights bit for bit"
    assert torch.equal(w, run(E.OPTIM_SGD)[0]), "sgd: bit-identical from run to run"
    if mode == "sum":
        fp, up = R64.widen_factor(ref["d_psw32"], ref["d_psw"])
        report(f"{name} d_psw", d_psw_f.cpu().numpy(), ref["d_psw"], up, fp)
        assert_close(d_psw_f.cpu().numpy(), ref["d_psw"], f"{name} d_psw under fused sgd", rtol=RTOL * fp, atol_scale=ATOL_SCALE * fp)
        assert torch.equal(d_psw_f, d_psw), "d_psw: the same from the dense route (the weights before the update)"
        _, row = DR.lookups(c["idx"], c["off"], c["base"], c["B"], pads)
        assert not d_psw_f.cpu().numpy()[row < 0].any(), "d_psw is 0 at padding"
    # ---- element-wise Adagrad from a live, all-distinct state
    w, s, _, _ = run(E.OPTIM_ADAGRAD, c["s_elem"])
    want_w, want_s = DR.adagrad(c["w"], c["s_elem"], ref["G"], touched, LR, EPS)
    gw, gs = w.cpu().numpy(), s.cpu().numpy()
    R64.assert_state_close(gs, want_s, ref["G"], f"{name} {mode} adagrad state", scale=f)
    assert_adagrad_close(gw, want_w, ref["G"], f"{name} {mode} adagrad weights", lr=LR, eps=EPS, state0=c["s_elem"], scale=f)
    assert np.array_equal(gw[~touched], c["w"][~touched]) and np.array_equal(gs[~touched], c["s_elem"][~touched]), \
        "adagrad: untouched rows keep weights and state bit for bit"
    w2, s2, _, _ = run(E.OPTIM_ADAGRAD, c["s_elem"])
    assert torch.equal(w, w2) and torch.equal(s, s2), "adagrad: bit-identical from run to run"
    # ---- row-wise Adagrad
    w, s, _, _ = run(E.OPTIM_ADAGRAD, c["s_row"])
    want_w, want_s = DR.rowwise_adagrad(c["w"], c["s_row"], ref["G"], touched, LR, EPS)
    gw, gs = w.cpu().numpy(), s.cpu().numpy()
    tol_w, tol_s = rowwise_bound(want_w, want_s, ref["G"], f, LR, EPS)
    assert_within(gs, want_s, tol_s, f"{name} {mode} row-wise state")
    assert_within(gw, want_w, tol_w, f"{name} {mode} row-wise weights")
    assert np.array_equal(gw[~touched], c["w"][~touched]) and np.array_equal(gs[~touched], c["s_row"][~touched])
    w2, s2, _, _ = run(E.OPTIM_ADAGRAD, c["s_row"])
    assert torch.equal(w, w2) and torch.equal(s, s2), "row-wise adagrad: bit-identical from run to run"


def test_cases_reach_what_they_are_for():
    """the shapes above against the sizes the library reports (no kernel runs)"""
    C = split_len()
    info = eng().dense_bags_info(64, 1000)
    assert info["one_launch"] == 0, "a one-launch route appeared: add batch sizes on both sides of its switch to CASES"
    for k, more in ((1, 0), (1, 1), (2, 0), (2, 1)):
        c = case(f"split_{k}_{more}")
        assert int((c["idx"][:c["off"][c["B"]]] == 0).sum()) == k * C + more
    c = case("d64")
    lens = np.diff(c["off"])
    assert lens.max() == 70 and not lens[2 * c["B"]:3 * c["B"]].any() and (lens == 0).sum() > c["B"]
    assert not reference("d64", "sum")["touched"][c["base"][2]:c["base"][3]].any()
    assert not reference("nnz0", "sum")["touched"].any() and not reference("all_padding", "sum")["touched"].any()
    assert case("d64_b1")["B"] == 1 and case("d3_b1")["D"] == 3 and case("d260")["D"] > 256


def test_sum_over_one_slot_bags_is_the_gathered_rows_bit_for_bit():
    c = case("d64")
    rs = np.random.RandomState(9)
    B, base = 37, c["base"]
    idx = np.concatenate([rs.randint(0, e, size=B) for e in c["Es"]]).astype(np.int64)
    rows = idx + np.repeat(base[:-1], B)
    for name in ("d64", "d64_misaligned", "d6"):
        cc = case(name)
        w = dev_weight(cc)
        out, _, _ = eng().dense_bags_forward(torch.from_numpy(idx).to(DEV), torch.arange(4 * B + 1, device=DEV), base.tolist(), w)
        assert torch.equal(out, w[torch.from_numpy(rows).to(DEV)]), name


def test_bad_indices_are_clamped_into_their_table():
    c = case("d64")
    w = dev_weight(c)
    idx = torch.tensor([7, 1 << 40, 24, 99999], device=DEV)
    out, _, _ = eng().dense_bags_forward(idx, torch.arange(5, device=DEV), c["base"].tolist(), w)
    assert torch.equal(out, w[torch.tensor([2, 3, 27, 1487], device=DEV)])


# ------------------------------------------------------------------------------------------------------------ the module
def _module(mode, optimizer, pads, sparse=True):
    import ttx_dense as TD

    torch.manual_seed(5)
    return TD.DenseTableBatchedEmbeddingBag(ES, 16, optimizer=optimizer, learning_rate=LR, eps=EPS, sparse=sparse, device=DEV, mode=mode,
                                            padding_idx=pads)


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_module_three_steps_equal_one_torch_embedding_bag_per_table(mode, opt):
    """Every step is checked on its own: both sides start it from the SAME trained weights and state (after the comparison the
    module takes torch's, so that the bound of a step need not carry the earlier steps' differences on rows this step leaves alone).
    Both sides are fp32, each within one bound of the exact result: two bounds apart at most (scale 2).  Adagrad starts from a live
    state (0.5) on both sides: from zero the first step divides by |g| + eps."""
    import ttx_dense as TD

    B, D, s0 = 9, 16, 0.5
    m = _module(mode, TD.OptimType.SGD if opt == "sgd" else TD.OptimType.EXACT_ADAGRAD, PADS)
    bags = [torch.nn.EmbeddingBag(e, D, mode=mode, padding_idx=p, include_last_offset=True).to(DEV) for e, p in zip(ES, PADS)]
    with torch.no_grad():
        for k, b in enumerate(bags):
            b.weight.copy_(m.table_weight(k))
        m.optimizer_state.fill_(s0)
    params = [b.weight for b in bags]
    o = torch.optim.SGD(params, lr=LR) if opt == "sgd" else torch.optim.Adagrad(params, lr=LR, eps=EPS, initial_accumulator_value=s0)
    state = np.full((sum(ES), D), s0)
    for step in range(3):
        idx, off, psw = DR.make_batch(40 + step, ES, B, pad=PADS, tie_table=2)
        d_out = torch.from_numpy(np.random.RandomState(50 + step).standard_normal((4, B, D)).astype(np.float32)).to(DEV)
        pw = torch.from_numpy(psw).to(DEV) if mode == "sum" else None
        out = m(torch.from_numpy(idx).to(DEV), torch.from_numpy(off).to(DEV), pw)
        assert out.shape == (4, B, D)
        o.zero_grad()
        touts = []
        for t, b in enumerate(bags):
            s, e = int(off[t * B]), int(off[(t + 1) * B])
            touts.append(b(torch.from_numpy(idx[s:e]).to(DEV), torch.from_numpy(off[t * B:(t + 1) * B + 1] - s).to(DEV),
                           None if pw is None else pw[s:e]))
        t_out = torch.stack(touts)
        scale = 2.0
        assert_close(out.detach().cpu().numpy(), t_out.detach().cpu().numpy(), f"{mode} {opt} step {step} forward", rtol=RTOL * scale,
                     atol_scale=ATOL_SCALE * scale)
        t_out.backward(d_out)
        G = torch.cat([b.weight.grad for b in bags]).cpu().numpy().astype(np.float64)
        out.backward(d_out)
        assert m.weight.grad is None, "sparse=True: the update is applied in backward, no weight gradient"
        o.step()
        want = torch.cat([b.weight.detach() for b in bags]).cpu().numpy().astype(np.float64)
        got = m.weight.detach().cpu().numpy()
        if opt == "sgd":
            assert_within(got, want, own_bound(want) * scale + LR * grad_bound(G, scale), f"{mode} sgd step {step}")
        else:
            assert_adagrad_close(got, want, G, f"{mode} adagrad step {step}", lr=LR, eps=EPS, state0=state, scale=scale)
            R64.assert_state_close(m.optimizer_state.cpu().numpy(), state + G * G, G, f"{mode} adagrad state step {step}", scale=scale)
            t_state = torch.cat([o.state[p]["sum"] for p in params])
            state = t_state.cpu().numpy().astype(np.float64)
            m.optimizer_state.copy_(t_state)
        with torch.no_grad():
            m.weight.copy_(torch.cat([b.weight.detach() for b in bags]))


def test_module_dense_route_and_weight_gradient():
    import ttx_dense as TD

    m = _module("sum", TD.OptimType.SGD, PADS, sparse=False)
    idx, off, psw = DR.make_batch(60, ES, 9, pad=PADS)
    pw = torch.from_numpy(psw).to(DEV).requires_grad_()
    d_out = np.random.RandomState(61).standard_normal((36, 16)).astype(np.float32)
    w0 = m.weight.detach().cpu().numpy()
    out = m(torch.from_numpy(idx).to(torch.int32).to(DEV), torch.from_numpy(off).to(torch.int32).to(DEV), pw)  # (int32 is widened)
    out.backward(torch.from_numpy(d_out).to(DEV).view(4, 9, 16))
    G, touched, d_psw = DR.row_grads(w0, idx, off, m.row_base, 9, d_out, "sum", PADS, psw)
    assert_close(m.weight.grad.cpu().numpy(), G, "sparse=False: weight.grad")
    assert np.array_equal(m.weight.detach().cpu().numpy(), w0), "sparse=False trains nothing itself"
    assert_close(pw.grad.cpu().numpy(), d_psw, "per_sample_weights.grad")
    # the fused route returns the weights' gradient too, from the weights before the update
    f = _module("sum", TD.OptimType.EXACT_ROWWISE_ADAGRAD, PADS)
    pw2 = torch.from_numpy(psw).to(DEV).requires_grad_()
    f(torch.from_numpy(idx).to(DEV), torch.from_numpy(off).to(DEV), pw2).backward(torch.from_numpy(d_out).to(DEV).view(4, 9, 16))
    assert torch.equal(pw2.grad, pw.grad) and f.weight.grad is None
    assert not np.array_equal(f.weight.detach().cpu().numpy(), w0) and float(f.optimizer_state.max()) > 0
    # the 2-D form
    two = torch.from_numpy(np.random.RandomState(62).randint(0, 3, size=(8, 3))).to(DEV)
    flat = m(two.reshape(-1), torch.arange(0, 25, 3, device=DEV))
    assert torch.equal(m(two), flat) and flat.shape == (4, 2, 16)


def test_module_state_dict_round_trip():
    import ttx_dense as TD

    a = _module("sum", TD.OptimType.EXACT_ADAGRAD, PADS)
    idx, off, _ = DR.make_batch(63, ES, 9, pad=PADS)
    i, o = torch.from_numpy(idx).to(DEV), torch.from_numpy(off).to(DEV)
    a(i, o).backward(torch.ones(4, 9, 16, device=DEV))
    sd = a.state_dict()
    assert list(sd) == ["weight", "optimizer_state"] and float(sd["optimizer_state"].max()) > 0
    b = _module("sum", TD.OptimType.EXACT_ADAGRAD, PADS)
    with torch.no_grad():
        b.weight.add_(1.0)
    b.load_state_dict(sd)
    assert torch.equal(a.weight, b.weight) and torch.equal(a.optimizer_state, b.optimizer_state)
    with torch.no_grad():
        assert torch.equal(a(i, o), b(i, o))
    bag = torch.nn.EmbeddingBag(24, 16).to(DEV)
    b.table_weight(2).copy_(bag.weight.detach())
    assert torch.equal(b.weight.detach()[4:28], bag.weight.detach())


def test_captured_step_replayed_over_two_batches_equals_the_eager_steps():
    import ttx_dense as TD

    B, L = 6, 4
    rs = np.random.RandomState(70)
    batches = []
    for k in range(2):  # 2-D batches [tables * B, L] with different padding
        b = np.concatenate([rs.randint(0, e, size=(B, L)) for e in ES]).astype(np.int64)
        for t, p in enumerate(PADS):
            if p is not None:
                rows = b[t * B:(t + 1) * B]
                rows[rs.rand(B, L) < (0.2 + 0.4 * k)] = p
        batches.append(torch.from_numpy(b).to(DEV))
    d_out = torch.from_numpy(rs.standard_normal((4, B, 16)).astype(np.float32)).to(DEV)
    eager = _module("mean", TD.OptimType.EXACT_ADAGRAD, PADS)
    graphed = _module("mean", TD.OptimType.EXACT_ADAGRAD, PADS)
    w0 = eager.weight.detach().clone()
    assert torch.equal(w0, graphed.weight.detach())
    eager_outs = []
    for b in batches:
        out = eager(b)
        out.backward(d_out)
        eager_outs.append(out.detach().clone())
    static = batches[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture's stream (workspace, cached offsets), then undo its training
        graphed(static).backward(d_out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        gout = graphed(static)
        gout.backward(d_out)
    torch.cuda.synchronize()
    with torch.no_grad():
        graphed.weight.copy_(w0)
        graphed.optimizer_state.zero_()
    for k, b in enumerate(batches):
        static.copy_(b)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(gout, eager_outs[k]), f"replay {k}: output"
    assert torch.equal(graphed.weight, eager.weight) and torch.equal(graphed.optimizer_state, eager.optimizer_state)


# ----------------------------------------------------------------------------------------------------- the mixed module
MIXED = [3, 200000, 1460, 24, 50000, 583]


def _mixed(**kw):
    import ttx_mixed as TM

    torch.manual_seed(11)
    kw.setdefault("fused", True)
    return TM.MixedTTEmbeddingBag(MIXED, 64, [8, 8], learning_rate=LR, device=DEV, include_last_offset=True, **kw)


def _mixed_batch(seed, B=8, pads=None):
    rs = np.random.RandomState(seed)
    idx, off = [], []
    for k, e in enumerate(MIXED):
        lens = rs.randint(0, 5, size=B)
        i = rs.randint(0, e, size=int(lens.sum()))
        if pads is not None and pads[k] is not None and i.size:
            i[rs.rand(i.size) < 0.3] = pads[k]
        idx.append(torch.from_numpy(i.astype(np.int64)).to(DEV))
        off.append(torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(DEV))
    return idx, off


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_mixed_dense_below(mode):
    pads = [1, 7, None, 5, 0, -1]
    m = _mixed(dense_below=10000, mode=mode, padding_idx=pads)
    assert m.dense_group_tables == [[0, 2, 3, 5]] and sorted(k for g in m.group_tables for k in g) == [1, 4]
    assert len(m.dense_groups) == 1 and m.dense_tables == [True, False, True, True, False, True]
    keys = list(m.state_dict())
    assert any(k.startswith("dense_groups.0.") for k in keys) and "dense_groups.0.weight" in keys
    idx, off = _mixed_batch(80, pads=m.padding_idx)
    outs = m(idx, off)
    assert len(outs) == 6 and all(o.shape == (8, 64) for o in outs)
    dg = m.dense_groups[0]
    for j, k in enumerate(m.dense_group_tables[0]):  # the caller's order: table k's own rows, torch's own pooling (fp32 both: 2 bounds)
        want = F.embedding_bag(idx[k], dg.table_weight(j), off[k], mode=mode, include_last_offset=True, padding_idx=m.padding_idx[k])
        assert_close(outs[k].detach().cpu().numpy(), want.cpu().numpy(), f"dense table {k}", rtol=2 * RTOL, atol_scale=2 * ATOL_SCALE)
    for mod, tables in zip(m.groups, m.group_tables):  # the TT tables: the group's own lookup of the same merged batch
        gi, go, gw = m._merge(tables, idx, off, None)
        res = mod(gi, go, True, gw).detach()
        for j, k in enumerate(tables):
            assert torch.equal(outs[k].detach(), res[j]), f"TT table {k}"
    before = dg.weight.detach().clone()
    cores = [c.detach().clone() for c in m.groups[0].tt_cores]
    torch.stack(outs).sum().backward()
    assert not torch.equal(before, dg.weight.detach()), "the dense tables train"
    assert any(not torch.equal(a, b.detach()) for a, b in zip(cores, m.groups[0].tt_cores)), "the TT tables train"


def test_mixed_per_sample_weights_and_2d_form():
    m = _mixed(dense_below=10000)
    rs = np.random.RandomState(81)
    idx = [torch.from_numpy(rs.randint(0, e, size=(8, 3)).astype(np.int64)).to(DEV) for e in MIXED]
    psw = [torch.from_numpy(rs.uniform(0.5, 1.5, size=(8, 3)).astype(np.float32)).to(DEV).requires_grad_() if k % 2 == 0 else None
           for k in range(6)]
    outs = m(idx, [None] * 6, psw)
    dg = m.dense_groups[0]
    for j, k in enumerate(m.dense_group_tables[0]):
        want = F.embedding_bag(idx[k], dg.table_weight(j), mode="sum", per_sample_weights=None if psw[k] is None else psw[k].detach())
        assert_close(outs[k].detach().cpu().numpy(), want.cpu().numpy(), f"dense table {k}", rtol=2 * RTOL, atol_scale=2 * ATOL_SCALE)
    w0 = dg.table_weight(0).clone()
    torch.stack(outs).sum().backward()
    want = w0[idx[0]].sum(dim=2)  # d/d psw of sum(out) = the looked-up row's sum, from the weights before the update
    assert_close(psw[0].grad.cpu().numpy(), want.cpu().numpy(), "per_sample_weights.grad of a dense table", rtol=2 * RTOL,
                 atol_scale=2 * ATOL_SCALE)


def test_mixed_defaults_are_unchanged():
    a, b = _mixed(), _mixed(dense_below=0)
    for m in (a, b):
        assert len(m.dense_groups) == 0 and m.dense_group_tables == [] and not any(m.dense_tables)
        assert sorted(k for g in m.group_tables for k in g) == list(range(6))
        assert not any("dense" in k for k in m.state_dict())
        want = [f"groups.{i}.{k}" for i, g in enumerate(m.groups) for k in g.state_dict()]
        assert list(m.state_dict()) == want, "the TT groups' keys and nothing else"
    assert list(a.state_dict()) == list(b.state_dict()) and a.group_tables == b.group_tables
    c = _mixed(dense=[False] * 6, dense_below=10 ** 9)
    assert c.group_tables == a.group_tables and len(c.dense_groups) == 0


def test_mixed_cache_with_dense_tables_populates_and_trains():
    m = _mixed(dense_below=10000, use_cache=True, cache_size=256, hashtbl_size=4096)
    assert all(g.use_cache for g in m.groups) and len(m.dense_groups) == 1
    assert sum(int(g.cache_weight.size(0)) for g in m.groups) <= 256, "the cache_size split sees the TT tables only"
    idx, off = _mixed_batch(82)
    m(idx, off)  # warm-up: counts the TT tables' keys
    m.cache_populate()
    assert all(not g.warmup for g in m.groups)
    before = [m.dense_groups[0].weight.detach().clone()] + [g.cache_weight.detach().clone() for g in m.groups]
    outs = m(idx, off)
    torch.stack(outs).sum().backward()
    torch.cuda.synchronize()
    assert not torch.equal(before[0], m.dense_groups[0].weight.detach())
    assert all(torch.isfinite(o).all() for o in outs)
    m.update_cache(idx, off)
    m.reset_cache()
