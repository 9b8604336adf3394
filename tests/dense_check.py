"""What tests/test_dense_tables_gpu.py and tests/test_dense_shapes_gpu.py share: the comparison of the kernels of
csrc/ttx_dense.hip with the float64 restatement tests/dense_ref.py on one case of tests/dense_cases.py (`check_kernels`), and the
bounds it uses.

Tolerance: the suite's default (tests/util.py: rtol 1e-5, atol 2e-6 max|ref|).  A comparison is widened only by the rule of
tests/test_fused_optimizer_gpu.py: when a plain fp32 numpy sum in index order of the same case (dense_ref with dtype=float32) is
itself more than half a default bound from float64, twice that distance is allowed, capped at (5e-5, 1e-5)
(tt_ref64.widen_factor).  Every figure is printed (pytest -s).  The updated weights are bounded by the gradient's bound carried
through the update: SGD is linear in G (lr dG); element-wise Adagrad as util.assert_adagrad_close(state0=, scale=) derives it; the
row-wise form by the same derivative with the row's state (rowwise_bound below)."""
import functools

import numpy as np
import torch

import dense_cases as DC
import dense_ref as DR
import tt_ref64 as R64
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

DEV = "cuda"
LEGS = ("forward", "dense", "sgd", "adagrad", "rowwise")


def eng():
    import tt_embeddings as E

    return E


def split_len():
    return eng().dense_bags_info(64, 1000)["split"]


def case(name):
    return DC.case(name, split_len())


def references(c, mode, vec=True):
    """float64 and plain-fp32 results of (case, mode); vec: the vectorised restatement (pinned to the loop forms bit for bit by
    tests/test_dense_tables_cpu.py), which the cases beyond a few thousand lookups need"""
    fwd, grads = (DR.forward_vec, DR.row_grads_vec) if vec else (DR.forward, DR.row_grads)
    psw = c["psw"] if mode == "sum" else None
    a = (c["w"], c["idx"], c["off"], c["base"], c["B"])
    out, live, arg = fwd(*a, mode, c["pads"], psw)
    out32, _, _ = fwd(*a, mode, c["pads"], psw, dtype=np.float32)
    G, touched, d_psw = grads(*a, c["d_out"], mode, c["pads"], psw)
    G32, _, d_psw32 = grads(*a, c["d_out"], mode, c["pads"], psw, dtype=np.float32)
    return dict(out=out, live=live, arg=arg, out32=out32, G=G, touched=touched, d_psw=d_psw, G32=G32, d_psw32=d_psw32, psw=psw)


@functools.lru_cache(maxsize=None)
def reference(name, mode, vec=False):
    """the same, computed once per (case, mode) and shared"""
    return references(case(name), mode, vec)


def off_by_one_float(shape):
    """a contiguous fp32 view of `shape` one float off a 16-byte boundary"""
    n = int(np.prod(shape))
    buf = torch.zeros(n + 1, device=DEV)
    v = buf[1:].view(*shape)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def dev_weight(c):
    """the case's weights on the device: 16-byte aligned, or -- misaligned -- a contiguous view one float off"""
    R, D = c["w"].shape
    if c.get("misaligned"):
        w = off_by_one_float((R, D))
    else:
        w = torch.empty((R, D), device=DEV)
        assert w.data_ptr() % 16 == 0
    w.copy_(torch.from_numpy(c["w"]))
    return w


def dev_like(a, misaligned=False):
    if not misaligned:
        t = torch.from_numpy(a).to(DEV)
        assert t.data_ptr() % 16 == 0
        return t
    t = off_by_one_float(a.shape)
    t.copy_(torch.from_numpy(a))
    return t


def batch(c, mode):
    psw = torch.from_numpy(c["psw"]).to(DEV) if mode == "sum" else None
    return torch.from_numpy(c["idx"]).to(DEV), torch.from_numpy(c["off"]).to(DEV), psw


def report(what, got, ref, u, f):
    k = R64.default_units(got, ref)
    print(f"[dense-tables] {what}: kernel {k:.3f}, plain fp32 {u:.3f} default bounds from float64 -> bound x{f:.2f}")
    return k


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


def check_kernels(name, mode, c, ref, legs=LEGS, figures=None):
    """the forward and the backward's four routes on case `c` against `ref` (references(c, mode)).  The forward always runs (the
    backward takes its live counts and argmax); legs: which of the backward's comparisons follow.  The case's flags misaligned /
    misaligned_d_out / misaligned_state put the weights / grad_output / the element-wise Adagrad state one float off a 16-byte
    boundary.  figures: a dict that receives the printed distances (kernel, plain fp32) per comparison."""
    E = eng()
    idx, off, psw = batch(c, mode)
    base, pads = c["base"].tolist(), c["pads"]
    w0 = dev_weight(c)
    d_out = dev_like(c["d_out"], c.get("misaligned_d_out", False))
    touched = ref["touched"]

    def note(what, got, want, u, f):
        k = report(f"{name} {mode} {what}", got, want, u, f)
        if figures is not None:
            figures[what] = (k, u)

    # ---- forward
    out, live, arg = E.dense_bags_forward(idx, off, base, w0, mode, pads, psw)
    got = out.cpu().numpy()
    if mode == "max":
        assert np.array_equal(got, ref["out"].astype(np.float32)), "max: the output is a selection -- exact"
        assert np.array_equal(arg.cpu().numpy(), ref["arg"]), "max: argmax"
    else:
        f, u = R64.widen_factor(ref["out32"], ref["out"])
        note("forward", got, ref["out"], u, f)
        assert_close(got, ref["out"], f"{name} {mode} forward", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    if mode == "mean":
        assert np.array_equal(live.cpu().numpy(), ref["live"])
    empty = ref["live"] == 0
    assert not got[empty].any(), "a bag without a live slot is exact zeros"
    out2, live2, arg2 = E.dense_bags_forward(idx, off, base, w0, mode, pads, psw)
    assert torch.equal(out, out2) and (arg is None or torch.equal(arg, arg2)), "forward: bit-identical from run to run"
    # ---- the dense gradient
    f, u = R64.widen_factor(ref["G32"], ref["G"])

    def run(optim, state=None, want=False, state_off=False):
        w = dev_weight(c)
        s = None if state is None else dev_like(state, state_off)
        d_w, d_psw = E.dense_bags_backward(optim, idx, off, base, w, d_out, mode, pads, psw, live, arg, LR, EPS, s, want)
        return w, s, d_w, d_psw

    d_psw = None
    if "dense" in legs:
        _, _, d_w, d_psw = run(E.OPTIM_DENSE, want=mode == "sum")
        gw = d_w.cpu().numpy()
        note("G", gw, ref["G"], u, f)
        assert_close(gw, ref["G"], f"{name} {mode} dense gradient", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
        assert not gw[~touched].any(), "dense: rows the batch does not touch are exactly zero"
        assert torch.equal(d_w, run(E.OPTIM_DENSE)[2]), "dense gradient: bit-identical from run to run"
    # ---- fused SGD, and the weights' gradient from the pre-update weights
    if "sgd" in legs:
        w, _, _, d_psw_f = run(E.OPTIM_SGD, want=mode == "sum")
        gw = w.cpu().numpy()
        want_w = DR.sgd(c["w"], ref["G"], touched, LR)
        assert_within(gw, want_w, own_bound(want_w) + LR * grad_bound(ref["G"], f), f"{name} {mode} sgd weights")
        assert np.array_equal(gw[~touched], c["w"][~touched]), "sgd: untouched rows keep their weights bit for bit"
        assert torch.equal(w, run(E.OPTIM_SGD)[0]), "sgd: bit-identical from run to run"
        if mode == "sum":
            fp, up = R64.widen_factor(ref["d_psw32"], ref["d_psw"])
            note("d_psw", d_psw_f.cpu().numpy(), ref["d_psw"], up, fp)
            assert_close(d_psw_f.cpu().numpy(), ref["d_psw"], f"{name} d_psw under fused sgd", rtol=RTOL * fp, atol_scale=ATOL_SCALE * fp)
            if d_psw is not None:
                assert torch.equal(d_psw_f, d_psw), "d_psw: the same from the dense route (the weights before the update)"
            _, row = DR.lookups_vec(c["idx"], c["off"], c["base"], c["B"], pads)
            assert not d_psw_f.cpu().numpy()[row < 0].any(), "d_psw is 0 at padding"
    # ---- element-wise Adagrad from a live, all-distinct state
    if "adagrad" in legs:
        so = c.get("misaligned_state", False)
        w, s, _, _ = run(E.OPTIM_ADAGRAD, c["s_elem"], state_off=so)
        want_w, want_s = DR.adagrad(c["w"], c["s_elem"], ref["G"], touched, LR, EPS)
        gw, gs = w.cpu().numpy(), s.cpu().numpy()
        R64.assert_state_close(gs, want_s, ref["G"], f"{name} {mode} adagrad state", scale=f)
        assert_adagrad_close(gw, want_w, ref["G"], f"{name} {mode} adagrad weights", lr=LR, eps=EPS, state0=c["s_elem"], scale=f)
        assert np.array_equal(gw[~touched], c["w"][~touched]) and np.array_equal(gs[~touched], c["s_elem"][~touched]), \
            "adagrad: untouched rows keep weights and state bit for bit"
        w2, s2, _, _ = run(E.OPTIM_ADAGRAD, c["s_elem"], state_off=so)
        assert torch.equal(w, w2) and torch.equal(s, s2), "adagrad: bit-identical from run to run"
    # ---- row-wise Adagrad
    if "rowwise" in legs:
        w, s, _, _ = run(E.OPTIM_ADAGRAD, c["s_row"])
        want_w, want_s = DR.rowwise_adagrad(c["w"], c["s_row"], ref["G"], touched, LR, EPS)
        gw, gs = w.cpu().numpy(), s.cpu().numpy()
        tol_w, tol_s = rowwise_bound(want_w, want_s, ref["G"], f, LR, EPS)
        assert_within(gs, want_s, tol_s, f"{name} {mode} row-wise state")
        assert_within(gw, want_w, tol_w, f"{name} {mode} row-wise weights")
        assert np.array_equal(gw[~touched], c["w"][~touched]) and np.array_equal(gs[~touched], c["s_row"][~touched])
        w2, s2, _, _ = run(E.OPTIM_ADAGRAD, c["s_row"])
        assert torch.equal(w, w2) and torch.equal(s, s2), "row-wise adagrad: bit-identical from run to run"
