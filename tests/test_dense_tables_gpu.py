"""GPU tests of the dense member tables: the kernels of csrc/ttx_dense.hip against the float64 restatement
tests/dense_ref.py at the smallest shapes that reach every path, `DenseTableBatchedEmbeddingBag` against one nn.EmbeddingBag per
table, and `MixedTTEmbeddingBag(dense_below=)`.

Tolerance: the suite's default (tests/util.py: rtol 1e-5, atol 2e-6 max|ref|).  A comparison is widened only by the rule of
tests/test_fused_optimizer_gpu.py: when a plain fp32 numpy sum in index order of the same case (dense_ref with dtype=float32) is
itself more than half a default bound from float64, twice that distance is allowed, capped at (5e-5, 1e-5)
(tt_ref64.widen_factor).  Every figure is printed (pytest -s).  The updated weights are bounded by the gradient's bound carried
through the update: SGD is linear in G (lr dG); element-wise Adagrad as util.assert_adagrad_close(state0=, scale=) derives it; the
row-wise form by the same derivative with the row's state (dense_check.rowwise_bound).

The cases are built by tests/dense_cases.py, the comparison itself is tests/dense_check.py::check_kernels, which
tests/test_dense_shapes_gpu.py runs on the shapes of the measured workload."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as DR
import tt_ref64 as R64
from dense_cases import ES, OLD_CASES as CASES, PADS
from dense_check import (DEV, assert_within, case, check_kernels, dev_weight, eng, grad_bound, own_bound, reference,  # noqa: F401
                         split_len)
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("name", CASES)
def test_kernels_against_float64(name, mode):
    check_kernels(name, mode, case(name), reference(name, mode))


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
