"""GPU tests of from_pretrained / truncate_ranks: TT-SVD and rounding with the table on the device (rocBLAS /
rocSOLVER under torch), and the modules they build on every route they take -- the HIP lookup kernels, the fused optimizers, the
row cache.  Expected numbers come from tests/svd_ref.py (float64 numpy); shapes, tables and tolerances are those of
tests/test_svd_cpu.py (see its docstring: exact-rank tables take all prod(p) rows, the padded rows are covered by the truncated
full-rank tables)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import svd_ref as R
from test_svd_cpu import EXACT, NAMES, TRUNC, VAR_P, exact_table, f64, full_rank_table, gapped_table, geometry, trunc_ref
from util import RTOL, assert_close

pytestmark = pytest.mark.gpu


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def ops():
    import tt_embeddings_ops

    return tt_embeddings_ops


def batch(E, seed=0, B_extra=9):
    """(indices, offsets) on the host: every row in a bag of its own, then B_extra bags of 1 .. 5 random lookups"""
    rs = np.random.RandomState(seed)
    lens = np.concatenate([np.ones(E, np.int64), 1 + np.arange(B_extra) % 5])
    idx = np.concatenate([np.arange(E), rs.randint(0, E, size=int(lens[E:].sum()))]).astype(np.int64)
    return torch.from_numpy(idx), torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))


def bag_ref(W, idx, off):
    """F.embedding_bag on the float64 table"""
    return F.embedding_bag(idx, torch.from_numpy(np.asarray(W, dtype=np.float64)), off, mode="sum", include_last_offset=True).numpy()


def batched(idx_off, n):
    """n tables' (indices, offsets) -> the table-major batch"""
    idx = torch.cat([i for i, _ in idx_off])
    off, base = [], 0
    for i, o in idx_off:
        off.append(o[:-1] + base)
        base += i.numel()
    return idx, torch.cat(off + [torch.tensor([base])])


# ------------------------------------------------------------------------------------------- forward through the HIP kernels
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", ["TTEmbeddingBag", "TTEmbedding"])
def test_exact_rank_table_forward(name, kind):
    p, q = geometry(name)
    ranks = R.CASES[name]["ranks"]
    _, W = exact_table(name)
    E = W.shape[0]
    cls = getattr(ops(), kind)
    m = cls.from_pretrained(t(W), ranks, p, q, device=dev(), use_cache=False)
    assert m.tt_ranks == [1] + ranks + [1] and m.tt_cores[0].is_cuda
    idx, off = batch(E, seed=1)
    if kind == "TTEmbedding":
        out = m(idx.to(dev()))
        ref = W.astype(np.float64)[idx.numpy()]
    else:
        out = m(idx.to(dev()), off.to(dev()))
        ref = bag_ref(W, idx, off)
    assert_close(out.detach().cpu().numpy(), ref, f"{kind} {name}: the ORIGINAL table")
    assert_close(m.full_weight(0).cpu().numpy(), W, f"{kind} {name}: full_weight")


def test_exact_rank_tables_forward_batched_var_and_mixed():
    import ttx_mixed

    O = ops()
    name = "T3"
    p, q = geometry(name)
    ranks = R.CASES[name]["ranks"]
    _, W = exact_table(name)
    both = [W, (W[::-1] * 0.5).copy()]
    m = O.TableBatchedTTEmbeddingBag.from_pretrained(t(np.stack(both)), ranks, p, q, device=dev())
    idx, off = batched([batch(60, seed=2), batch(60, seed=3)], 2)
    out = m(idx.to(dev()), off.to(dev())).detach().cpu().numpy()
    for k, (i, o) in enumerate((batch(60, seed=2), batch(60, seed=3))):
        assert_close(out[k], bag_ref(both[k], i, o), f"batched table {k}")
    # tables of different row factors: [3, 4, 5] (60 rows) and [2, 5, 4] (40 rows), exact ranks [4, 3] over all their rows
    W40 = R.tt_full(R.random_cores(np.random.RandomState(40), VAR_P[1], q, ranks)).astype(np.float32)
    m = ttx_mixed.VarTableTTEmbeddingBag.from_pretrained([t(W), t(W40)], ranks, VAR_P, q, device=dev())
    pairs = [batch(60, seed=4, B_extra=29), batch(40, seed=5, B_extra=49)]  # (the same number of bags)
    idx, off = batched(pairs, 2)
    out = m(idx.to(dev()), off.to(dev())).detach().cpu().numpy()
    for k, (w, (i, o)) in enumerate(zip((W, W40), pairs)):
        assert_close(out[k], bag_ref(w, i, o), f"var table {k}")
        assert_close(m.full_weight(k).cpu().numpy(), w, f"var full_weight {k}")
    # mixed: one dense member (E = 7) beside two TT members of different p
    small = np.random.RandomState(3).standard_normal((7, 24)).astype(np.float32)
    tables = [W, small, W40]
    for fused in (False, True):
        m = ttx_mixed.MixedTTEmbeddingBag.from_pretrained([t(w) for w in tables], ranks, [VAR_P[0], None, VAR_P[1]], q, device=dev(),
                                                          fused=fused, dense_below=10, include_last_offset=True)
        assert m.dense_tables == [False, True, False] and m.compression[1] is None
        pairs = [batch(60, seed=6, B_extra=29), batch(7, seed=7, B_extra=82), batch(40, seed=8, B_extra=49)]
        outs = m([i.to(dev()) for i, _ in pairs], [o.to(dev()) for _, o in pairs])
        for k, (w, (i, o)) in enumerate(zip(tables, pairs)):
            assert_close(outs[k].detach().cpu().numpy(), bag_ref(w, i, o), f"mixed (fused={fused}) table {k}")
        assert torch.equal(m.full_weight(1).cpu(), torch.from_numpy(small))


@pytest.mark.parametrize("name", NAMES)
def test_truncated_table_forward(name):
    p, q = geometry(name)
    W, ref = full_rank_table(name), trunc_ref(name)
    E = W.shape[0]
    m = ops().TTEmbeddingBag.from_pretrained(t(W), TRUNC[name], p, q, device=dev(), use_cache=False)
    idx, off = batch(E, seed=9)
    rows = m(idx.to(dev()), off.to(dev())).detach().cpu().numpy()[:E]
    err = float(np.linalg.norm(rows.astype(np.float64) - W))
    err_ref = float(np.linalg.norm(R.tt_full(ref["cores"], E) - W))
    print(f"{name}: error of the looked-up rows {err:.6f}, restatement {err_ref:.6f}, norm {ref['norm']:.4f}")
    assert abs(err - err_ref) <= RTOL * ref["norm"]
    np.testing.assert_allclose(m.compression[0][1:], [ref["bound"], ref["norm"]], rtol=1e-6)
    # the restatement's float64 cores, loaded: the forward is their table
    m.load_table_cores([t(c) for c in R.pad_ranks(ref["cores"], TRUNC[name])])
    out = m(idx.to(dev()), off.to(dev())).detach().cpu().numpy()
    assert_close(out, bag_ref(R.tt_full(ref["cores"], E), idx, off), f"{name}: the restatement's cores")


# ------------------------------------------------------------------------------------------------------------ training step
@pytest.mark.parametrize("optimizer", ["EXACT_SGD", "EXACT_ADAM"])
@pytest.mark.parametrize("kind,name", [("TTEmbeddingBag", "T3"), ("TTEmbeddingBag", "T2"), ("TTEmbeddingBag", "T4"),
                                       ("TTEmbeddingBag", "cap"), ("TableBatchedTTEmbeddingBag", "T3")])
def test_a_compressed_module_trains_like_its_constructor_built_twin(kind, name, optimizer):
    O = ops()
    p, q = geometry(name)
    ranks = R.CASES[name]["ranks"]
    _, W = exact_table(name)
    E, D = W.shape
    kw = dict(device=dev(), optimizer=getattr(O.OptimType, optimizer), learning_rate=0.05, eps=1e-4)
    if kind == "TTEmbeddingBag":
        a = O.TTEmbeddingBag.from_pretrained(t(W), ranks, p, q, use_cache=False, **kw)
        b = O.TTEmbeddingBag(E, D, ranks, p, q, use_cache=False, **kw)
        idx, off = batch(E, seed=11)
    else:
        a = O.TableBatchedTTEmbeddingBag.from_pretrained(t(np.stack([W, W * 0.5])), ranks, p, q, **kw)
        b = O.TableBatchedTTEmbeddingBag(2, E, D, ranks, p, q, **kw)
        idx, off = batched([batch(E, seed=11), batch(E, seed=12)], 2)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict())
    idx, off = idx.to(dev()), off.to(dev())
    start = [c.detach().clone() for c in a.tt_cores]
    outs = []
    for m in (a, b):
        out = m(idx, off)
        outs.append(out.detach().clone())
        grad = torch.from_numpy(np.random.RandomState(13).standard_normal(tuple(out.shape)).astype(np.float32)).to(dev())
        out.backward(grad)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    for c0, ca, cb in zip(start, a.tt_cores, b.tt_cores):
        assert not torch.equal(ca.detach(), c0), "the step moved the cores"
        assert torch.equal(ca.detach(), cb.detach()), "bit-identical cores after the step"
    sa, sb = a.state_dict(), b.state_dict()
    for key, v in sa.items():  # (the optimizer's state too)
        assert torch.equal(v, sb[key]), key


# -------------------------------------------------------------------------------------------------------------------- cache
def test_cached_module_from_pretrained():
    name = "T3"
    p, q = geometry(name)
    _, W = exact_table(name)
    m = ops().TTEmbeddingBag.from_pretrained(t(W), R.CASES[name]["ranks"], p, q, device=dev(), use_cache=True, cache_size=16,
                                             sparse=False)
    assert m.use_cache and m.warmup, "a cache starts in warm-up"
    rs = np.random.RandomState(17)
    hot = torch.from_numpy(rs.randint(0, 20, size=200).astype(np.int64)).to(dev())
    m(hot, torch.arange(0, 201, 4, device=dev()))  # warm-up: counted
    idx, off = batch(60, seed=18)
    idx, off = idx.to(dev()), off.to(dev())
    uncached = m(idx, off).detach().cpu().numpy()
    m.cache_populate()
    assert not m.warmup and int((m.cache_state >= 0).sum()) > 0
    live = m(idx, off).detach().cpu().numpy()
    assert_close(live, uncached, "live cache against the uncached forward")
    assert_close(live, bag_ref(W, idx.cpu(), off.cpu()), "live cache against the original table")


# ------------------------------------------------------------------------------------------------------------ device parity
@pytest.mark.parametrize("route", ["svd", "gram"])
@pytest.mark.parametrize("name", NAMES)
def test_device_side_factorisation_equals_the_cpu_call(monkeypatch, name, route):
    import ttx_svd

    if route == "gram":
        monkeypatch.setattr(ttx_svd, "_SVD_DIRECT_MAX", 0)
    p, q = geometry(name)
    W = full_rank_table(name)
    norm = trunc_ref(name)["norm"]
    on_dev, on_cpu = ttx_svd.tt_svd(t(W), p, q, TRUNC[name]), ttx_svd.tt_svd(torch.from_numpy(W), p, q, TRUNC[name])
    assert all(c.is_cuda and c.dtype == torch.float32 for c in on_dev.cores)
    errs = [R.error(W, f64([c.cpu() for c in r.cores])) for r in (on_dev, on_cpu)]
    print(f"{name} {route}: error on the device {errs[0]:.6f}, on the CPU {errs[1]:.6f}, restatement {R.error(W, trunc_ref(name)['cores']):.6f}")
    assert on_dev.ranks == on_cpu.ranks == TRUNC[name]
    assert abs(errs[0] - errs[1]) <= RTOL * norm
    assert abs(errs[0] - R.error(W, trunc_ref(name)["cores"])) <= RTOL * norm
    np.testing.assert_allclose(on_dev.eps_k, trunc_ref(name)["eps_k"], rtol=1e-6)
    G = gapped_table(name)
    chosen_dev, chosen_cpu = ttx_svd.tt_svd(t(G), p, q, rel_error=1e-2), ttx_svd.tt_svd(torch.from_numpy(G), p, q, rel_error=1e-2)
    assert chosen_dev.ranks == chosen_cpu.ranks == EXACT[name]
    cores, _ = exact_table(name, tuple(EXACT[name]))
    lower = [max(1, r - 1) for r in EXACT[name]]
    full = R.tt_full(cores)
    rounded = ttx_svd.tt_round([t(c) for c in cores], lower)
    ref = R.tt_svd(full, p, q, lower)
    assert abs(R.error(full, f64([c.cpu() for c in rounded.cores])) - R.error(full, ref["cores"])) <= RTOL * ref["norm"]


# ----------------------------------------------------------------------------------------------------------- truncate_ranks
@pytest.mark.parametrize("kind", ["TTEmbeddingBag", "TableBatchedTTEmbeddingBag"])
def test_truncate_ranks_on_the_device(kind):
    O = ops()
    name = "T3"
    p, q = geometry(name)
    cores, W = exact_table(name)
    full = R.tt_full(cores)
    ref = R.tt_svd(full, p, q, [2, 2])
    table = R.tt_full(ref["cores"])
    if kind == "TTEmbeddingBag":
        m = O.TTEmbeddingBag.from_pretrained(t(W), [4, 3], p, q, device=dev(), use_cache=False)
        scales, (idx, off) = [1.0], batch(60, seed=21)
    else:
        m = O.TableBatchedTTEmbeddingBag.from_pretrained(t(np.stack([W, W * 0.5])), [4, 3], p, q, device=dev())
        scales, (idx, off) = [1.0, 0.5], batched([batch(60, seed=21), batch(60, seed=22)], 2)
    low = m.truncate_ranks([2, 2])
    assert low.tt_ranks == [1, 2, 2, 1] and low.tt_cores[0].is_cuda and low._ctor_kwargs() == m._ctor_kwargs()
    out = low(idx.to(dev()), off.to(dev())).detach().cpu().numpy().reshape(len(scales), -1, 24)
    for k, (s, (i, o)) in enumerate(zip(scales, (batch(60, seed=21), batch(60, seed=22)))):
        assert_close(out[k], bag_ref(table * s, i, o), f"{kind} table {k}: the restatement's rounded cores")
