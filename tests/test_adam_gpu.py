"""GPU tests of the fused Adam: `ttx_adam_apply` against the float64 restatement tests/adam_ref.py on identical
fp32 inputs, a captured call against eager calls, and OptimType.EXACT_ADAM on every family of lookup routes against adam_ref fed
the float64 gradient of tests/tt_ref64.py (dense member tables: tests/dense_ref.py).

Tolerances.  Kernel against restatement: the suite's default (util.RTOL, util.ATOL_SCALE) -- the gradient is the same on both
sides.  Modules: the gradient's default bound dg = ATOL_SCALE max|g| + RTOL |g| carried through the update's derivative
(adam_ref.weight_tolerance / moment_tolerances, the rule of util.assert_adagrad_close).  dg is widened only by the rule of
tests/test_fused_optimizer_gpu.py: when the fp32 oracle's dense gradient of the same case is itself more than half a default bound
from float64, twice that distance, capped at 5 (tt_ref64.widen_factor).  Every figure is printed (pytest -s).

The reference takes the hyper-parameters as the C ABI carries them: rounded to float (adam_ref.f32)."""
import os
import re

import numpy as np
import pytest
import torch

import adam_ref as AR
import dense_ref as DR
import gen_inputs as G
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, RTOL, assert_close

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETAS = (0.9, 0.999)
WD = 0.05


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def eng():
    import tt_embeddings as E

    return E


def _source_constants():
    """the kernel's walk, read off csrc/ttx_adam.hip (as tests/dense_cases.py mirrors ttx_dense.hip)"""
    src = open(os.path.join(ROOT, "fbtt-embedding_amd", "csrc", "ttx_adam.hip")).read()
    val = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))  # noqa: E731
    return val("kAdamGridCap"), val("kAdamT"), val("kAdamVec")


GRID_CAP, BLOCK, VEC = _source_constants()
SWEEP = GRID_CAP * BLOCK * VEC  # elements of one full grid sweep


def hyper(wd_mode):
    wd = 0.0 if wd_mode == "none" else WD
    f = AR.f32
    return dict(lr=f(LR), betas=(f(BETAS[0]), f(BETAS[1])), eps=f(EPS), weight_decay=f(wd), decoupled=wd_mode == "decoupled")


# ---- a live state for one tensor ----------------------------------------------------------------------------------------------------
def live_tensor(rs, n, zero_block=True):
    """fp32 (w, g, m, v) of n elements: every element of each array distinct; half of v LARGE (4 .. 6 max g^2: the step is dominated
    by the prior state), half SMALL (1e-3 .. 1.5e-3 max g^2: dominated by the gradient); one block with m = v = g = 0.
    -> (w, g, m, v, slice of the zero block)"""
    if n == 0:
        e = np.zeros(0, dtype=np.float32)
        return e, e.copy(), e.copy(), e.copy(), slice(0, 0)

    def distinct(scale, signed=True):
        x = (rs.permutation(n) + 1.0) / (n + 1.0)
        x = x * (np.where(rs.rand(n) < 0.5, -1.0, 1.0) if signed else 1.0)
        return (scale * x).astype(np.float32)

    w, g, m = distinct(1.0), distinct(0.3), distinct(0.2)
    m2 = max(float((g.astype(np.float64) ** 2).max()), 1e-12)
    frac = (rs.permutation(n) + 1.0) / (n + 1.0)
    v = np.where(rs.rand(n) < 0.5, 4.0 * m2 * (1.0 + 0.5 * frac), 1e-3 * m2 * (1.0 + 0.5 * frac)).astype(np.float32)
    if n > 1:
        assert np.unique(v).size == n and np.unique(w).size == n and np.unique(g).size == n and np.unique(m).size == n
    zb = slice(0, 0)
    if zero_block and n >= 4:
        zb = slice(n // 3, n // 3 + max(1, n // 4))
        g[zb] = 0.0
        m[zb] = 0.0
        v[zb] = 0.0
    return w, g, m, v, zb


KERNEL_CASES = {
    # name: [(numel, offset in floats of the view into its buffer)]
    "one": [(1027, 0)],
    "three_with_empty": [(257, 0), (0, 0), (1027, 0)],
    "four_misaligned": [(3 * BLOCK * VEC + 5, 1), (256, 0), (2 * BLOCK * VEC, 1), (5, 1)],
    "sixteen": [(n, 0) for n in (1, 3, 4, 5, 255, 256, 257, 1027, 0, BLOCK * VEC, 2 * BLOCK * VEC, BLOCK * VEC + 1, 7, 0,
                                 4 * BLOCK * VEC + 3, 64)],
    "beyond_one_sweep": [(SWEEP + 5, 0), (300, 0)],
}


def _run_kernel(case, step0, wd_mode, seed=0):
    """-> (inputs as numpy, outputs as numpy, step after)"""
    rs = np.random.RandomState(1000 + seed)
    E, h = eng(), hyper(wd_mode)
    ins, views = [], []
    for n, shift in KERNEL_CASES[case]:
        w, g, m, v, zb = live_tensor(rs, n)
        ins.append((w, g, m, v, zb))
        four = []
        for a in (w, g, m, v):
            buf = torch.zeros(n + shift + 4, dtype=torch.float32, device=dev())
            view = buf[shift:shift + n]
            view.copy_(torch.from_numpy(a))
            if n:
                assert (view.data_ptr() % 16 == 0) == (shift == 0)
            four.append(view)
        views.append(four)
    step = torch.tensor([step0], dtype=torch.int64, device=dev())
    E.adam_apply([f[0] for f in views], [f[1] for f in views], [f[2] for f in views], [f[3] for f in views], step, h["lr"],
                 h["betas"], h["eps"], h["weight_decay"], h["decoupled"])
    torch.cuda.synchronize()
    outs = [tuple(x.cpu().numpy() for x in f) for f in views]
    return ins, outs, int(step.item())


@pytest.mark.parametrize("wd_mode", ["none", "coupled", "decoupled"])
@pytest.mark.parametrize("step0", [0, 1, 1000])
@pytest.mark.parametrize("case", ["one", "three_with_empty", "four_misaligned", "sixteen"])
def test_kernel_against_float64(case, step0, wd_mode):
    _check_kernel(case, step0, wd_mode)


@pytest.mark.parametrize("wd_mode,step0", [("none", 1000), ("coupled", 0), ("decoupled", 1)])
def test_kernel_beyond_one_grid_sweep(wd_mode, step0):
    assert KERNEL_CASES["beyond_one_sweep"][0][0] == GRID_CAP * BLOCK * 4 + 5
    _check_kernel("beyond_one_sweep", step0, wd_mode)


def _check_kernel(case, step0, wd_mode):
    h = hyper(wd_mode)
    ins, outs, step_after = _run_kernel(case, step0, wd_mode)
    assert step_after == step0 + 1
    for k, ((w, g, m, v, zb), (gw, gg, gm, gv)) in enumerate(zip(ins, outs)):
        rw, rm, rv, rt = AR.step(w, g, m, v, step0, **h)
        assert rt == step_after
        assert np.array_equal(gg, g), f"{case}[{k}]: the gradient was written"
        assert_close(gw, rw, f"{case}[{k}] w")
        assert_close(gm, rm, f"{case}[{k}] exp_avg")
        assert_close(gv, rv, f"{case}[{k}] exp_avg_sq")
        if wd_mode == "none":  # m = v = g = 0: the element does not move, bit for bit
            assert np.array_equal(gw[zb], w[zb]) and not gm[zb].any() and not gv[zb].any(), f"{case}[{k}]: the zero block moved"
    ins2, outs2, _ = _run_kernel(case, step0, wd_mode)
    for a, b in zip(outs, outs2):
        assert all(np.array_equal(x, y) for x, y in zip(a, b)), f"{case}: two runs from the same inputs differ"


def test_nothing_to_step_leaves_the_counter():
    E = eng()
    step = torch.tensor([5], dtype=torch.int64, device=dev())
    z = torch.zeros(0, device=dev())
    E.adam_apply([], [], [], [], step, 0.1, BETAS, 1e-8)
    E.adam_apply([z, z], [z, z], [z, z], [z, z], step, 0.1, BETAS, 1e-8)
    assert int(step.item()) == 5
    with pytest.raises(RuntimeError):
        E.adam_apply([z] * 17, [z] * 17, [z] * 17, [z] * 17, step, 0.1, BETAS, 1e-8)


def test_captured_call_replayed_equals_eager_calls():
    """one adam_apply captured in a hipGraph and replayed three times == three eager calls, bit for bit: the step lives on the
    device and the replay advances it"""
    E, h = eng(), hyper("coupled")
    rs = np.random.RandomState(7)
    data = [live_tensor(rs, n, zero_block=False) for n in (1027, 0, 3 * BLOCK * VEC + 1)]

    def fresh():
        return [[t(a) for a in d[:4]] for d in data], torch.zeros(1, dtype=torch.int64, device=dev())

    def call(ts, step):
        E.adam_apply([f[0] for f in ts], [f[1] for f in ts], [f[2] for f in ts], [f[3] for f in ts], step, h["lr"], h["betas"],
                     h["eps"], h["weight_decay"], h["decoupled"])

    ea, es = fresh()
    for _ in range(3):
        call(ea, es)
    ga, gs = fresh()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call(ga, gs)
    assert int(gs.item()) == 0, "capturing is not running"
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(es.item()) == int(gs.item()) == 3
    for a, b in zip(ea, ga):
        for j, name in enumerate(("w", "g", "exp_avg", "exp_avg_sq")):
            assert torch.equal(a[j], b[j]), name


# ---- the modules ----------------------------------------------------------------------------------------------------------------------
def _dg(g64, scale=1.0):
    g = np.abs(np.asarray(g64, dtype=np.float64))
    return scale * (ATOL_SCALE * max(float(g.max()) if g.size else 0.0, 1e-30) + RTOL * g)


def live_moments(rs, g64):
    """fp32 (exp_avg, exp_avg_sq) to start a step from: distinct elements, half of v dominated by the prior state and half by
    the gradient (tt_ref64.live_state's rule), m of the gradient's size with either sign"""
    g64 = np.asarray(g64, dtype=np.float64)
    n = g64.size
    m2 = max(float((g64 * g64).max()), 1e-12)
    frac = (rs.permutation(n) + 1.0) / (n + 1.0)
    v = np.where(rs.rand(n) < 0.5, 4.0 * m2 * (1.0 + 0.5 * frac), 1e-3 * m2 * (1.0 + 0.5 * frac)).astype(np.float32)
    m = (np.sqrt(m2) * 0.5 * ((rs.permutation(n) + 1.0) / (n + 1.0)) * np.where(rs.rand(n) < 0.5, -1.0, 1.0)).astype(np.float32)
    return m.reshape(g64.shape), v.reshape(g64.shape)


def check_step(what, w0, g64, m0, v0, step0, got_w, got_m, got_v, h, scale=1.0):
    """every element of the weights and the two moments after ONE step against adam_ref fed the float64 gradient"""
    rw, rm, rv, _ = AR.step(w0, g64, m0, v0, step0, **h)
    dg = _dg(g64, scale).reshape(rw.shape)
    tol_w = AR.weight_tolerance(rw, rm, rv, g64, dg, step0 + 1, h["lr"], h["betas"], h["eps"], RTOL)
    tol_m, tol_v = AR.moment_tolerances(rm, rv, g64, dg, h["betas"], m0)
    for name, got, ref, tol in (("w", got_w, rw, tol_w), ("exp_avg", got_m, rm, tol_m), ("exp_avg_sq", got_v, rv, tol_v)):
        got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
        assert np.isfinite(got).all(), f"{what} {name}: non-finite"
        err = np.abs(got - ref)
        print(f"{what} {name}: worst error / bound = {float((err / tol).max()):.3f} (scale {scale:.2f})")
        bad = err > tol
        if bad.any():
            i = np.unravel_index(np.argmax(err - tol), err.shape)
            raise AssertionError(f"{what} {name}: {int(bad.sum())}/{bad.size} out of tolerance; worst at {i}: got {got[i]!r} "
                                 f"ref {ref[i]!r} tol {tol[i]:.3e}")


def _bags(seed, tables, B, E, pad=None, max_len=6):
    """ragged table-major bags, a fifth of them empty; `pad` sprinkled in, one bag of padding only"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(1, max_len + 1, size=tables * B) * (rs.rand(tables * B) > 0.2)
    lens[0] = max(lens[0], 2)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rs.randint(0, E, size=int(off[-1])).astype(np.int64)
    if pad is not None:
        idx[rs.rand(idx.size) < 0.15] = pad
        idx[off[0]:off[1]] = pad
    return idx, off


def _reference_gradient(c, cores, idx, off, d_out, psw=None, mode="sum", pad=None):
    """-> (float64 core gradients, widening scale per core) of the batch as the module sees it"""
    tables, B = c["tables"], (off.size - 1) // c["tables"]
    keep = np.ones(idx.size, dtype=bool) if pad is None else idx != pad
    before = np.concatenate([[0], np.cumsum(keep)])
    off2, idx2 = before[off], idx[keep]
    rowidx, tableidx = R.rowidx_from_offsets(off2, tables)
    w = None if psw is None else np.asarray(psw, dtype=np.float64)[keep]
    if mode == "mean":
        lens = np.diff(off2)
        w = 1.0 / np.maximum(lens, 1)[tableidx * B + rowidx]
    res = R.forward_backward(tables, c["p"], c["q"], c["r"], B, idx2, rowidx, tableidx, cores, d_out, per_sample_weights=w)
    scales = [1.0] * len(cores)
    if not isinstance(c["p"][0], (list, tuple)):  # the fp32 oracle's dense gradient of the same case: the yardstick of a widening
        ones = np.ones(idx2.size, dtype=np.float32) if w is None else w.astype(np.float32)
        og = R.oracle_on_restatement(tables, c["p"], c["q"], c["r"], B, idx2, rowidx, tableidx, ones, cores, d_out, LR)[2]
        for k, (o, g) in enumerate(zip(og, res["grads"])):
            scales[k], u = R.widen_factor(o, g)
            print(f"  core {k}: the fp32 oracle is {u:.3f} default bounds from float64 -> scale {scales[k]:.2f}")
    return res["grads"], scales


def _tt_module(c, **kw):
    import tt_embeddings_ops as ops

    m = ops.TableBatchedTTEmbeddingBag(c["tables"], int(np.prod(c["p"])), int(np.prod(c["q"])), c["r"][1:-1], c["p"], c["q"],
                                       optimizer=ops.OptimType.EXACT_ADAM, learning_rate=LR, eps=EPS, weight_dist="uniform",
                                       use_cache=False, device=dev(), **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, c["cores"]):
            dst.copy_(t(src))
    return m


def _shape(tables, p, q, ranks, seed):
    r = [1] + list(ranks) + [1]
    return dict(tables=tables, p=list(p), q=list(q), r=r, cores=G.make_cores(seed, tables, p, q, r, "signed"))


def _seed_state(m, rs, grads, step0):
    m0v0 = [live_moments(rs, g) for g in grads]
    with torch.no_grad():
        for k, (a, b) in enumerate(m0v0):
            m.optimizer_state[k].copy_(t(a))
            m.optimizer_state_v[k].copy_(t(b))
        m.optimizer_step.fill_(step0)
    return m0v0


TT_CASES = {
    # name: (tables, p, q, ranks, B, module keywords, forward: psw?, what the route must be)
    "padded_generic": (1, [7, 9, 11], [3, 4, 5], [13, 12], 40, {}, False),
    "template": (1, [10, 9, 11], [4, 4, 4], [32, 32], 60, {}, False),
    "two_cores": (1, [9, 40], [8, 8], [32], 50, {}, False),
    "four_cores": (1, [7, 9, 11, 5], [3, 4, 5, 7], [13, 12, 7], 30, {}, False),
    "part_lookups": (1, [5, 6, 7], [12, 4, 4], [16, 16], 50, {}, False),
    "padded_core0": (2, [5, 6, 7], [7, 4, 4], [16, 16], 40, {}, False),
    "two_tables": (2, [7, 9, 11], [3, 4, 5], [13, 12], 40, {}, False),
    "dedup": (2, [7, 9, 11], [3, 4, 5], [13, 12], 40, dict(dedup=True), False),
    "mean": (2, [7, 9, 11], [3, 4, 5], [13, 12], 40, dict(mode="mean"), False),
    "padding_idx": (2, [7, 9, 11], [3, 4, 5], [13, 12], 40, dict(padding_idx=5), False),
    "per_sample_weights": (2, [10, 9, 11], [4, 4, 4], [32, 32], 40, {}, True),
}


@pytest.mark.parametrize("step0", [0, 7])
@pytest.mark.parametrize("name", list(TT_CASES))
def test_module_step_against_float64(name, step0):
    tables, p, q, ranks, B, kw, weighted = TT_CASES[name]
    c = _shape(tables, p, q, ranks, 31)
    E, D = int(np.prod(p)), int(np.prod(q))
    h = hyper("coupled" if name in ("template", "two_tables") else "none")
    m = _tt_module(c, betas=BETAS, weight_decay=h["weight_decay"], **kw)
    if name == "part_lookups":
        assert m._split0 > 1 and not m._pad0, "the geometry is expected to run as part lookups"
    if name == "padded_core0":
        assert m._pad0 == 8 and m._split0 == 2, "core 0 is expected to be zero-padded"
    pad = kw.get("padding_idx")
    idx, off = _bags(41, tables, B, E, pad)
    assert idx.size <= 2000 and (np.diff(off) == 0).any()
    d_out = G.make_grad(43, tables, B, D)
    psw = np.random.RandomState(44).uniform(0.5, 1.5, size=idx.size).astype(np.float32) if weighted else None
    grads, scales = _reference_gradient(c, c["cores"], idx, off, d_out, psw, kw.get("mode", "sum"), pad)
    m0v0 = _seed_state(m, np.random.RandomState(45), grads, step0)
    out = m(t(idx), t(off), per_sample_weights=None if psw is None else t(psw))
    out.backward(t(d_out))
    torch.cuda.synchronize()
    assert all(cr.grad is None for cr in m.tt_cores) and int(m.optimizer_step.item()) == step0 + 1
    for k in range(len(p)):
        check_step(f"{name} core {k}", c["cores"][k], grads[k], m0v0[k][0], m0v0[k][1], step0, m.tt_cores[k].detach().cpu().numpy(),
                   m.optimizer_state[k].cpu().numpy(), m.optimizer_state_v[k].cpu().numpy(), h, scales[k])


@pytest.mark.parametrize("step0", [0, 7])
@pytest.mark.parametrize("pad", [None, 5])
def test_unpooled_module_step_against_float64(pad, step0):
    import tt_embeddings_ops as ops

    c = _shape(1, [7, 9, 11], [3, 4, 5], [13, 12], 51)
    E, D, h = 7 * 9 * 11, 60, hyper("decoupled")
    m = ops.TTEmbedding(E, D, [13, 12], c["p"], c["q"], optimizer=ops.OptimType.EXACT_ADAM, learning_rate=LR, eps=EPS,
                        weight_dist="uniform", device=dev(), padding_idx=pad, weight_decay=WD, decoupled_weight_decay=True)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, c["cores"]):
            dst.copy_(t(src))
    rs = np.random.RandomState(52)
    idx = rs.randint(0, E, size=(9, 13)).astype(np.int64)
    if pad is not None:
        idx[rs.rand(*idx.shape) < 0.2] = pad
    d_out = rs.standard_normal((1, idx.size, D)).astype(np.float32)
    grads, scales = _reference_gradient(c, c["cores"], idx.reshape(-1), np.arange(idx.size + 1, dtype=np.int64), d_out, pad=pad)
    m0v0 = _seed_state(m, rs, grads, step0)
    m(t(idx)).backward(t(d_out.reshape(idx.shape + (D,))))
    torch.cuda.synchronize()
    assert all(cr.grad is None for cr in m.tt_cores) and int(m.optimizer_step.item()) == step0 + 1
    for k in range(3):
        check_step(f"unpooled core {k}", c["cores"][k], grads[k], m0v0[k][0], m0v0[k][1], step0, m.tt_cores[k].detach().cpu().numpy(),
                   m.optimizer_state[k].cpu().numpy(), m.optimizer_state_v[k].cpu().numpy(), h, scales[k])


@pytest.mark.parametrize("step0", [0, 7])
def test_mixed_module_with_a_dense_table(step0):
    """MixedTTEmbeddingBag(fused=True, dense_below=): two TT tables of different row factors in one group, one dense table; one
    Adam step per group"""
    import tt_embeddings_ops as ops
    import ttx_mixed

    Es, D, q, ranks, B = [24, 7 * 9 * 11, 6 * 9 * 10], 60, [3, 4, 5], [13, 12], 30
    ps = [None, [7, 9, 11], [6, 9, 10]]
    h = hyper("coupled")
    torch.manual_seed(61)
    m = ttx_mixed.MixedTTEmbeddingBag(Es, D, ranks, ps, q, optimizer=ops.OptimType.EXACT_ADAM, learning_rate=LR, eps=EPS,
                                      weight_dist="uniform", device=dev(), include_last_offset=True, fused=True, dense_below=100,
                                      weight_decay=WD)
    assert m.dense_group_tables == [[0]] and m.group_tables == [[1, 2]] and len(m.groups) == 1
    tt, dn = m.groups[0], m.dense_groups[0]
    rs = np.random.RandomState(62)
    with torch.no_grad():
        for cr in tt.tt_cores:
            cr.copy_(t(rs.uniform(-0.5, 0.5, size=tuple(cr.shape)).astype(np.float32)))
    batches = [_bags(63 + k, 1, B, e) for k, e in enumerate(Es)]
    d_out = rs.standard_normal((3, B, D)).astype(np.float32)
    # references: the TT group (tables 1, 2 table-major) and the dense table
    cores0 = [cr.detach().cpu().numpy().copy() for cr in tt.tt_cores]
    c = dict(tables=2, p=[ps[1], ps[2]], q=q, r=[1] + ranks + [1])
    idx_tt = np.concatenate([batches[1][0], batches[2][0]])
    off_tt = np.concatenate([batches[1][1], batches[2][1][1:] + batches[1][1][-1]])
    grads, scales = _reference_gradient(c, cores0, idx_tt, off_tt, d_out[1:])
    w0 = dn.weight.detach().cpu().numpy().copy()
    Gd, _, _ = DR.row_grads(w0, batches[0][0], batches[0][1], [0, Es[0]], B, d_out[0])
    sd, ud = R.widen_factor(DR.row_grads(w0, batches[0][0], batches[0][1], [0, Es[0]], B, d_out[0], dtype=np.float32)[0], Gd)
    print(f"  dense table: a plain fp32 sum is {ud:.3f} default bounds from float64 -> scale {sd:.2f}")
    mv_tt = _seed_state(tt, rs, grads, step0)
    md, vd = live_moments(rs, Gd)
    with torch.no_grad():
        dn.optimizer_state.copy_(t(md))
        dn.optimizer_state_v.copy_(t(vd))
        dn.optimizer_step.fill_(step0)
    outs = m([t(b[0]) for b in batches], [t(b[1]) for b in batches])
    torch.autograd.backward(outs, [t(d_out[k]) for k in range(3)])
    torch.cuda.synchronize()
    assert int(tt.optimizer_step.item()) == int(dn.optimizer_step.item()) == step0 + 1
    assert dn.weight.grad is None and all(cr.grad is None for cr in tt.tt_cores)
    for k in range(3):
        check_step(f"mixed core {k}", cores0[k], grads[k], mv_tt[k][0], mv_tt[k][1], step0, tt.tt_cores[k].detach().cpu().numpy(),
                   tt.optimizer_state[k].cpu().numpy(), tt.optimizer_state_v[k].cpu().numpy(), h, scales[k])
    check_step("mixed dense table", w0, Gd, md, vd, step0, dn.weight.detach().cpu().numpy(), dn.optimizer_state.cpu().numpy(),
               dn.optimizer_state_v.cpu().numpy(), h, sd)


# ---- further checks -------------------------------------------------------------------------------------------------------------------
def test_the_step_consumes_exactly_the_dense_gradient():
    """a second module with sparse=False gives, from the same inputs, the gradient the Adam module consumed: after step 1 from a
    zero state exp_avg == (1 - beta1) g within one rounding, and exp_avg_sq == (1 - beta2) g^2"""
    import tt_embeddings_ops as ops

    c = _shape(2, [10, 9, 11], [4, 4, 4], [32, 32], 71)
    E, D, B = 990, 64, 50
    a = _tt_module(c)
    b = ops.TableBatchedTTEmbeddingBag(2, E, D, [32, 32], c["p"], c["q"], sparse=False, weight_dist="uniform", use_cache=False,
                                       device=dev())
    with torch.no_grad():
        for dst, src in zip(b.tt_cores, c["cores"]):
            dst.copy_(t(src))
    idx, off = _bags(72, 2, B, E)
    d_out = t(G.make_grad(73, 2, B, D))
    a(t(idx), t(off)).backward(d_out)
    b(t(idx), t(off)).backward(d_out)
    omb1, omb2 = np.float32(1.0 - float(np.float32(BETAS[0]))), np.float32(1.0 - float(np.float32(BETAS[1])))
    for k in range(3):
        g = b.tt_cores[k].grad.cpu().numpy()
        m1, v1 = a.optimizer_state[k].cpu().numpy(), a.optimizer_state_v[k].cpu().numpy()
        assert g.any() and np.array_equal(m1 == 0, g == 0)
        np.testing.assert_allclose(m1, omb1 * g, rtol=2e-7, atol=0)
        np.testing.assert_allclose(v1, omb2 * g * g, rtol=4e-7, atol=1e-44)


def test_captured_training_step_replayed_equals_eager():
    """three eager steps of TableBatchedTTEmbeddingBag(EXACT_ADAM) == one captured step replayed three times, bit for bit"""
    c = _shape(2, [10, 9, 11], [4, 4, 4], [32, 32], 81)
    E, D, B = 990, 64, 50
    idx, off = _bags(82, 2, B, E)
    ti, to, d_out = t(idx), t(off), t(G.make_grad(83, 2, B, D))

    def one_step(m):
        m(ti, to).backward(d_out)

    a, b = _tt_module(c, weight_decay=WD), _tt_module(c, weight_decay=WD)
    for _ in range(3):
        one_step(a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # (a warm-up step off the default stream, as torch asks before a capture; then back to the start)
        one_step(b)
    torch.cuda.current_stream().wait_stream(side)
    with torch.no_grad():
        for k, src in enumerate(c["cores"]):
            b.tt_cores[k].copy_(t(src))
            b.optimizer_state[k].zero_()
            b.optimizer_state_v[k].zero_()
        b.optimizer_step.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        one_step(b)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert int(a.optimizer_step.item()) == int(b.optimizer_step.item()) == 3
    for k in range(3):
        assert torch.equal(a.tt_cores[k].detach(), b.tt_cores[k].detach()), f"core {k}"
        assert torch.equal(a.optimizer_state[k], b.optimizer_state[k]) and torch.equal(a.optimizer_state_v[k], b.optimizer_state_v[k])
        assert b.tt_cores[k].grad is None


def test_mixed_module_on_group_streams_joins_the_adam_step():
    """MixedTTEmbeddingBag(streams=True): every group's backward -- the Adam step behind the lookup's included -- runs on the
    group's stream and is joined to the caller's.  Two groups, two eager steps against the same module without streams, bit for
    bit; then one step captured (a capture refuses work that is not joined) and replayed against a third eager step."""
    import tt_embeddings_ops as ops
    import ttx_graph
    import ttx_mixed

    D, q, r, B = 12, [2, 3, 2], [4, 5], 16
    Es, ps = [100, 700, 90], [[4, 5, 5], [8, 9, 10], [4, 5, 5]]

    def make(streams):
        torch.manual_seed(95)
        return ttx_mixed.MixedTTEmbeddingBag(Es, D, r, ps, q, optimizer=ops.OptimType.EXACT_ADAM, learning_rate=LR, eps=EPS,
                                             weight_dist="uniform", device=dev(), include_last_offset=True, streams=streams)

    a, b = make(True), make(False)
    assert a.group_tables == [[0, 2], [1]] and a._streams is not None and b._streams is None
    batches = [[_bags(96 + 3 * k + j, 1, B, e) for j, e in enumerate(Es)] for k in range(3)]
    grads = [t(G.make_grad(97, 1, B, D)[0]) for _ in Es]

    def step(m, k):
        torch.autograd.backward(m([t(x[0]) for x in batches[k]], [t(x[1]) for x in batches[k]]), grads)

    def same(what):
        torch.cuda.synchronize()
        for ga, gb in zip(a.groups, b.groups):
            assert int(ga.optimizer_step.item()) == int(gb.optimizer_step.item())
            for k in range(3):
                assert torch.equal(ga.tt_cores[k].detach(), gb.tt_cores[k].detach()), f"{what}: core {k}"
                assert torch.equal(ga.optimizer_state[k], gb.optimizer_state[k]) and torch.equal(ga.optimizer_state_v[k], gb.optimizer_state_v[k])

    for k in range(2):
        step(a, k)
        step(b, k)
        same(f"eager step {k}")
    keep = {k: v.clone() for k, v in a.state_dict().items()}
    idx, off = [t(x[0]) for x in batches[2]], [t(x[1]) for x in batches[2]]
    rnd = ttx_graph.GraphedRound(lambda: torch.autograd.backward(a(idx, off), grads), [()], warmup=1)
    a.load_state_dict(keep)  # (the warm-up step in front of the capture moved the state: back to where step 2 starts, in place)
    rnd.replay()
    step(b, 2)
    same("captured step")


def test_set_learning_rate_and_empty_batch():
    c = _shape(1, [7, 9, 11], [3, 4, 5], [13, 12], 91)
    m = _tt_module(c)
    idx, off = _bags(92, 1, 20, 693)
    d_out = t(G.make_grad(93, 1, 20, 60))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    out = m(torch.zeros(0, dtype=torch.int64, device=dev()), torch.zeros(21, dtype=torch.int64, device=dev()))
    out.backward(d_out)
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in before.items()) and all(cr.grad is None for cr in m.tt_cores)
    m.set_learning_rate(0.0)
    m(t(idx), t(off)).backward(d_out)
    assert all(torch.equal(m.tt_cores[k].detach(), before[f"tt_cores.{k}"]) for k in range(3)) and int(m.optimizer_step.item()) == 1
    m.set_learning_rate(LR)
    m(t(idx), t(off)).backward(d_out)
    assert not any(torch.equal(m.tt_cores[k].detach(), before[f"tt_cores.{k}"]) for k in range(3))
