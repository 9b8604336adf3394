"""GPU tests of the dense member tables (csrc/ttx_dense.hip) at the run lengths and sizes of the measured workload
-- 16 tables x B 2048 x 20 slots: 32,768 bags, rows looked up thousands of times -- which tests/test_dense_tables_gpu.py stops short
of.  The cases (tests/dense_cases.py) are the smallest that reach each path; tests/test_dense_tables_cpu.py computes from numpy
alone what each of them reaches (run lengths and where the runs sit in the sorted order, the sort's pass count, lane layout, bags
per wave, slots per trip), pins the vectorised float64 reference used here to the loop forms of tests/dense_ref.py, and checks that
every case's plain-fp32 yardstick stays under the cap of the widening rule.

The comparison is tests/dense_check.py::check_kernels, the one test_dense_tables_gpu.py runs: forward, argmax and live exact,
run-to-run bit identity, the dense gradient, untouched rows exactly zero / unchanged, fused SGD, d_psw from the pre-update weights,
element-wise Adagrad from a live all-distinct state (all distinct at every size here: the largest state holds 1.12 M values below
113, apart by 1e-4), row-wise Adagrad.  Tolerances: the suite's default, widened only by that file's rule; no new number.
Measured distances of the long runs: profiles/r16_dense_shapes.md."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_cases as DC
import dense_ref as DR
import tt_ref64 as R64
from dense_check import DEV, assert_within, case, check_kernels, eng, grad_bound, own_bound, references, rowwise_bound
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
MODES = ["sum", "mean", "max"]


def test_split_length_is_the_mirrors():
    """the cases are sized by the split length the library reports; the CPU suite checks them at the mirror's"""
    assert eng().dense_bags_info(64, 1000) == {"split": DC.SPLIT, "one_launch": 0}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", DC.NEW_CASES)
def test_kernels_against_float64(name, mode):
    c = case(name)
    check_kernels(name, mode, c, references(c, mode))


def test_key_kernel_grid_stride_and_runs_of_a_thousand_chunks():
    """nnz = 2^21 + 300 > 8192 x 256 positions: sum mode; forward, dense gradient, fused SGD (and d_psw)"""
    c = case("keys_stride")
    assert c["idx"].size == DC.KEYS_NNZ and c["legs"] == ("forward", "dense", "sgd")
    check_kernels("keys_stride", "sum", c, references(c, "sum"), legs=c["legs"])


@pytest.mark.parametrize("what", ["d_out", "state"])
def test_misaligned_cases_put_the_forward_and_the_backward_on_different_routes(what):
    """(what the two alignment cases rely on: the views really are one float off, the weights are not)"""
    from dense_check import dev_like, dev_weight

    c = case(f"misaligned_{what}")
    assert dev_weight(c).data_ptr() % 16 == 0 and DC.layout(c["D"], True)[0] == 4 and DC.layout(c["D"], False)[0] == 1
    a = c["d_out"] if what == "d_out" else c["s_elem"]
    t = dev_like(a, True)
    assert t.data_ptr() % 16 == 4 and t.is_contiguous() and np.array_equal(t.cpu().numpy(), a)


# ----------------------------------------------------------------------------------------------------- the mixed module
MIXED = [3, 200000, 1460, 24, 50000, 583]
MIXED_PADS = [1, 7, None, 5, 0, -1]


def _mixed(num_embeddings=MIXED, **kw):
    import ttx_mixed as TM

    torch.manual_seed(11)
    kw.setdefault("fused", True)
    return TM.MixedTTEmbeddingBag(num_embeddings, 64, [8, 8], learning_rate=LR, eps=EPS, device=DEV, include_last_offset=True, **kw)


def _mixed_batch(seed, Es, B, pads):
    """per table: numpy (indices, offsets), 0-4 slots a bag, the table's padding value in about a third of the slots"""
    rs = np.random.RandomState(seed)
    idx, off = [], []
    for k, e in enumerate(Es):
        lens = rs.randint(0, 5, size=B)
        i = rs.randint(0, e, size=int(lens.sum())).astype(np.int64)
        if pads is not None and pads[k] is not None and i.size:
            i[rs.rand(i.size) < 0.3] = pads[k]
        idx.append(i)
        off.append(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    return idx, off


def _group_batch(tables, idx, off, pads):
    """the table-major batch of one dense group as the reference takes it: the tables' batches one after the other, a table's
    padding value rewritten to -1 (the merged batches' sentinel)"""
    gi, go, at = [], [np.zeros(1, np.int64)], 0
    for k in tables:
        i = idx[k].copy()
        if pads[k] is not None:
            i[i == pads[k]] = -1
        gi.append(i)
        go.append(off[k][1:] + at)
        at += i.size
    return np.concatenate(gi), np.concatenate(go)


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
@pytest.mark.parametrize("mode", MODES)
def test_mixed_dense_below_one_training_step(mode, opt):
    """One step of MixedTTEmbeddingBag(dense_below=10000) on a padded batch under a fixed random cotangent: the dense group's
    weight and optimizer_state against dense_ref applied to the group's tables -- the pre-step weights, the group's batch, the
    d_out autograd delivers (the cotangent itself) -- at the bounds of check_kernels.  Adagrad starts from a live state."""
    from ttx_dense import OptimType

    B, D = 8, 64
    m = _mixed(dense_below=10000, mode=mode, padding_idx=MIXED_PADS,
               optimizer=OptimType.SGD if opt == "sgd" else OptimType.EXACT_ADAGRAD)
    assert m.dense_group_tables == [[0, 2, 3, 5]] and len(m.dense_groups) == 1
    dg, tables = m.dense_groups[0], m.dense_group_tables[0]
    R = dg.weight.size(0)
    s0 = None
    if opt == "adagrad":
        s0 = (0.5 + 1e-4 * np.arange(R * D)).reshape(R, D).astype(np.float32)
        with torch.no_grad():
            dg.optimizer_state.copy_(torch.from_numpy(s0))
    w0 = dg.weight.detach().cpu().numpy().copy()
    idx, off = _mixed_batch(90, MIXED, B, m.padding_idx)
    assert all((idx[k] == m.padding_idx[k]).any() for k in tables if m.padding_idx[k] is not None), "the batch holds padding"
    cot = np.random.RandomState(91).standard_normal((len(MIXED), B, D)).astype(np.float32)
    outs = m([torch.from_numpy(i).to(DEV) for i in idx], [torch.from_numpy(o).to(DEV) for o in off])
    (torch.stack(outs) * torch.from_numpy(cot).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    gi, go = _group_batch(tables, idx, off, m.padding_idx)
    a = (w0, gi, go, np.asarray(dg.row_base, np.int64), B)
    d_out = cot[tables].reshape(len(tables) * B, D)
    out, _, _ = DR.forward_vec(*a, mode)
    out32, _, _ = DR.forward_vec(*a, mode, dtype=np.float32)
    got = torch.stack([outs[k] for k in tables]).detach().cpu().numpy().reshape(out.shape)
    f, u = R64.widen_factor(out32, out)
    if mode == "max":
        assert np.array_equal(got, out.astype(np.float32))
    else:
        assert_close(got, out, f"mixed {mode} forward", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    G, touched, _ = DR.row_grads_vec(*a, d_out, mode)
    G32, _, _ = DR.row_grads_vec(*a, d_out, mode, dtype=np.float32)
    f, u = R64.widen_factor(G32, G)
    print(f"[dense-tables] mixed {mode} {opt}: plain fp32 {u:.3f} default bounds from float64 -> bound x{f:.2f}")
    assert touched.any() and not touched.all()
    gw = dg.weight.detach().cpu().numpy()
    if opt == "sgd":
        want_w = DR.sgd(w0, G, touched, LR)
        assert_within(gw, want_w, own_bound(want_w) + LR * grad_bound(G, f), f"mixed {mode} sgd weights")
        assert dg.optimizer_state.numel() == 0
    else:
        want_w, want_s = DR.adagrad(w0, s0, G, touched, LR, EPS)
        gs = dg.optimizer_state.cpu().numpy()
        R64.assert_state_close(gs, want_s, G, f"mixed {mode} adagrad state", scale=f)
        assert_adagrad_close(gw, want_w, G, f"mixed {mode} adagrad weights", lr=LR, eps=EPS, state0=s0, scale=f)
        assert np.array_equal(gs[~touched], s0[~touched])
    assert np.array_equal(gw[~touched], w0[~touched]), "untouched rows keep their weights bit for bit"


def test_mixed_rowwise_adagrad_one_training_step():
    """the same under the row-wise state (one mode: the state's layout is the module's choice, not the pooling's)"""
    from ttx_dense import OptimType

    B, D, mode = 8, 64, "mean"
    m = _mixed(dense_below=10000, mode=mode, padding_idx=MIXED_PADS, optimizer=OptimType.EXACT_ROWWISE_ADAGRAD)
    dg, tables = m.dense_groups[0], m.dense_group_tables[0]
    R = dg.weight.size(0)
    s0 = (0.5 + 1e-3 * np.arange(R)).astype(np.float32)
    with torch.no_grad():
        dg.optimizer_state.copy_(torch.from_numpy(s0))
    w0 = dg.weight.detach().cpu().numpy().copy()
    idx, off = _mixed_batch(92, MIXED, B, m.padding_idx)
    cot = np.random.RandomState(93).standard_normal((len(MIXED), B, D)).astype(np.float32)
    outs = m([torch.from_numpy(i).to(DEV) for i in idx], [torch.from_numpy(o).to(DEV) for o in off])
    (torch.stack(outs) * torch.from_numpy(cot).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    gi, go = _group_batch(tables, idx, off, m.padding_idx)
    a = (w0, gi, go, np.asarray(dg.row_base, np.int64), B)
    d_out = cot[tables].reshape(len(tables) * B, D)
    G, touched, _ = DR.row_grads_vec(*a, d_out, mode)
    f, _ = R64.widen_factor(DR.row_grads_vec(*a, d_out, mode, dtype=np.float32)[0], G)
    want_w, want_s = DR.rowwise_adagrad(w0, s0, G, touched, LR, EPS)
    tol_w, tol_s = rowwise_bound(want_w, want_s, G, f, LR, EPS)
    gw, gs = dg.weight.detach().cpu().numpy(), dg.optimizer_state.cpu().numpy()
    assert_within(gs, want_s, tol_s, "mixed row-wise state")
    assert_within(gw, want_w, tol_w, "mixed row-wise weights")
    assert np.array_equal(gw[~touched], w0[~touched]) and np.array_equal(gs[~touched], s0[~touched])


@pytest.mark.parametrize("mode", MODES)
def test_mixed_seventy_dense_tables_are_two_groups(mode):
    """70 dense tables (cardinalities cycling through 1..7) beside one TT table: two dense groups of 64 and 6 tables, two merge
    launches; every table's output against torch's own pooling of that table's rows (fp32 both: 2 bounds)"""
    Es = [1 + k % 7 for k in range(70)] + [50000]
    pads = [(e - 1 if e > 1 and k % 4 == 1 else None) for k, e in enumerate(Es)]
    m = _mixed(Es, dense=[True] * 70 + [False], mode=mode, padding_idx=pads)
    assert [len(g) for g in m.dense_group_tables] == [64, 6] and m.dense_group_tables[1] == list(range(64, 70))
    assert sorted(k for g in m.group_tables for k in g) == [70]
    idx, off = _mixed_batch(94, Es, 3, m.padding_idx)
    ti, to = [torch.from_numpy(i).to(DEV) for i in idx], [torch.from_numpy(o).to(DEV) for o in off]
    outs = m(ti, to)
    assert len(outs) == 71 and all(o.shape == (3, 64) for o in outs)
    for dg, tables in zip(m.dense_groups, m.dense_group_tables):
        for j, k in enumerate(tables):
            want = F.embedding_bag(ti[k], dg.table_weight(j), to[k], mode=mode, include_last_offset=True, padding_idx=m.padding_idx[k])
            assert_close(outs[k].detach().cpu().numpy(), want.cpu().numpy(), f"dense table {k}", rtol=2 * RTOL, atol_scale=2 * ATOL_SCALE)
    before = [dg.weight.detach().clone() for dg in m.dense_groups]
    torch.stack(outs).sum().backward()
    assert all(not torch.equal(b, dg.weight.detach()) for b, dg in zip(before, m.dense_groups)), "both groups train"
