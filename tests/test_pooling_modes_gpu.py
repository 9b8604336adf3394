"""GPU tests of nn.EmbeddingBag's mean / max pooling modes on the TT bags (TTEmbeddingBag / TableBatchedTTEmbeddingBag
`mode=`): the new kernels against numpy through the C ABI, the module against torch's own embedding_bag on the expanded
table (forward, dense core gradients, fused SGD / Adagrad steps), ties, the cache-live and n_dev routes of mean, capture,
determinism and the refusals."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_inputs as G
from util import EPS, LR, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (name, p, q, ranks): two cores, the shape-specialised kernels, padded ranks, four cores, q0 = 8 (part lookups for sum / mean)
GEOMS = [
    ("t2", [5, 8], [3, 4], [6]),
    ("spec", [200, 220, 250], [4, 4, 4], [32, 32]),
    ("padded", [7, 9, 11], [3, 4, 5], [13, 12]),
    ("t4", [4, 5, 3, 4], [4, 4, 4, 4], [32, 32, 32]),
    ("q8", [10, 12, 14], [8, 4, 4], [16, 16]),
]
GEOM_IDS = [g[0] for g in GEOMS]


def use_route(route, monkeypatch):
    """"native": the sum lookup under mean runs as the C++ node; "python": as TTLookupFunction (max has this route only)"""
    import tt_embeddings_ops as ops

    if route == "python":
        monkeypatch.setenv("TTX_NO_NATIVE_NODE", "1")
        assert ops._native_node() is None
    else:
        monkeypatch.delenv("TTX_NO_NATIVE_NODE", raising=False)
        assert ops._native_node() is not None, "ttx_torch.so not built / not importable on this box"
    return route


@pytest.fixture(params=["native", "python"])
def node(request, monkeypatch):
    """the mean mode wraps the sum lookup: run it through the C++ node and through TTLookupFunction"""
    return use_route(request.param, monkeypatch)


MODE_ROUTES = [("mean", "native"), ("mean", "python"), ("max", "python")]


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- references
def np_max_pool(rows, off):
    nb, D = off.size - 1, rows.shape[1]
    out = np.zeros((nb, D), np.float32)
    arg = np.full((nb, D), -1, np.int32)
    for b in range(nb):
        s, e = int(off[b]), int(off[b + 1])
        if e > s:
            out[b] = rows[s:e].max(0)
            arg[b] = s + rows[s:e].argmax(0)  # (numpy: the first of equal maxima)
    return out, arg


def np_max_pool_backward(d_out, arg, off, nnz):
    d_rows = np.zeros((nnz, d_out.shape[1]), np.float32)
    for b in range(off.size - 1):
        for n in range(int(off[b]), int(off[b + 1])):
            hit = arg[b] == n
            d_rows[n, hit] = d_out[b, hit]
    return d_rows


def tt_rows_torch(p, q, ranks, cores_k, idx):
    """the TT rows of `idx` from one table's cores ([p_t, r_t q_t r_t+1] each), differentiable: the same product
    tt_matrix_to_full expands, for the looked-up rows only"""
    T = len(p)
    r = [1] + list(ranks) + [1]
    idx = torch.as_tensor(idx, device=DEV, dtype=torch.int64)
    n = idx.numel()
    digits, rest = [], idx
    for s in reversed(range(T)):
        digits.append(rest % p[s])
        rest = rest // p[s]
    digits = digits[::-1]
    acc = cores_k[0][digits[0]].reshape(n, q[0], r[1])
    for s in range(1, T):
        sl = cores_k[s][digits[s]].reshape(n, r[s], q[s] * r[s + 1])
        acc = torch.bmm(acc, sl).reshape(n, -1, r[s + 1])
    return acc.reshape(n, -1)


def ref_lookup(p, q, ranks, cores, idx, off, num_tables, mode):
    """[num_tables, B, D] = torch.nn.functional.embedding_bag(mode=...) of each table's bags on its TT rows"""
    B = (off.size - 1) // num_tables
    outs = []
    for k in range(num_tables):
        o = off[k * B:(k + 1) * B + 1].astype(np.int64)
        s, e = int(o[0]), int(o[-1])
        rows = tt_rows_torch(p, q, ranks, [c[k] for c in cores], idx[s:e])
        outs.append(F.embedding_bag(torch.arange(e - s, device=DEV), rows, t(o - s), mode=mode, include_last_offset=True))
    return torch.stack(outs)


def batch(seed, num_tables, B, E, long_bag=300):
    """bags of 0..8 lookups, one empty and one long bag per table (table-major) -> (indices, offsets with closing entry)"""
    rs = np.random.RandomState(seed)
    lengths = rs.randint(0, 9, size=num_tables * B)
    lengths[::B] = 0
    lengths[1::B] = long_bag
    lengths[2::B] = 1
    idx = rs.randint(0, E, size=int(lengths.sum())).astype(np.int64)
    return idx, np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def module(p, q, r, cores, num_tables, mode, **kw):
    import tt_embeddings_ops as ops

    kw.setdefault("use_cache", False)
    m = ops.TableBatchedTTEmbeddingBag(num_tables, int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform",
                                       device=DEV, mode=mode, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(t(src))
    return m


# ------------------------------------------------------------------------------------------------- kernels through the C ABI
@pytest.mark.parametrize("D", [3, 64, 128, 1024])
def test_max_pool_and_mean_scale_kernels_vs_numpy(D):
    import tt_embeddings as E

    rs = np.random.RandomState(D)
    lengths = np.array([0, 1, 5000, 3, 0, 17, 1, 64, 2, 200, 0])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    nnz = int(off[-1])
    rows = rs.standard_normal((nnz, D)).astype(np.float32)
    rows[:, ::2] = rs.randint(-2, 3, size=(nnz, (D + 1) // 2)) / 4.0  # every other column: a handful of levels -- ties everywhere
    out, arg = E.bag_max_pool(t(rows), t(off))
    ref_out, ref_arg = np_max_pool(rows, off)
    assert np.array_equal(arg.cpu().numpy(), ref_arg), "argmax: the first position of the bag's maxima"
    assert np.array_equal(out.cpu().numpy(), ref_out)
    assert (ref_arg[lengths == 0] == -1).all() and (out.cpu().numpy()[lengths == 0] == 0).all()
    d_out = rs.standard_normal((off.size - 1, D)).astype(np.float32)
    d_rows = E.bag_max_pool_backward(t(d_out), arg, t(off), nnz).cpu().numpy()
    assert np.array_equal(d_rows, np_max_pool_backward(d_out, ref_arg, off, nnz))
    assert (np.count_nonzero(d_rows, axis=0) <= (lengths > 0).sum()).all()  # one winner per bag and column
    x = rs.standard_normal((off.size - 1, D)).astype(np.float32)
    y = E.bag_mean_scale(t(x), t(off)).cpu().numpy()
    assert np.array_equal(y, x / np.maximum(lengths, 1).astype(np.float32)[:, None]), "mean scale (empty bags: divided by 1)"


@pytest.mark.parametrize("D", [3, 64])
def test_max_pool_backward_writes_every_row_once(D):
    """through the raw C ABI into a buffer full of NaN: lookups before offsets[0] / from offsets[nb] on get zero rows, all
    others the gather form -- nothing of the NaN survives (no memset is needed in front)"""
    import tt_embeddings as E

    rs = np.random.RandomState(7)
    off = np.array([2, 2, 5, 9, 30], np.int64)  # (positions 0, 1 and 30..39 belong to no bag)
    nnz = 40
    rows = rs.standard_normal((nnz, D)).astype(np.float32)
    out, arg = E.bag_max_pool(t(rows), t(off))
    d_out = rs.standard_normal((off.size - 1, D)).astype(np.float32)
    d_rows = torch.full((nnz, D), float("nan"), device=DEV)
    dev_out, dev_off = t(d_out), t(off)
    rc = E.lib().ttx_bag_max_pool_backward(off.size - 1, D, nnz, dev_off.data_ptr(), arg.data_ptr(), dev_out.data_ptr(),
                                           d_rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    got = d_rows.cpu().numpy()
    assert np.isfinite(got).all()
    assert np.array_equal(got, np_max_pool_backward(d_out, np_max_pool(rows, off)[1], off, nnz))


# ------------------------------------------------------------------------------------------------------ module: forward
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("mode,route", MODE_ROUTES, ids=[f"{m}-{r}" for m, r in MODE_ROUTES])
def test_forward_matches_torch_embedding_bag(geom, mode, route, monkeypatch):
    """3 tables, an empty / a one-lookup / a 300-lookup bag per table; both offset forms, int32 indices"""
    import tt_embeddings_ops as ops

    use_route(route, monkeypatch)
    _, p, q, r = geom
    nt, B, E_ = 3, 19, int(np.prod(p))
    cores = G.make_cores(21, nt, p, q, r, "signed")
    idx, off = batch(5, nt, B, E_)
    ref = ref_lookup(p, q, r, [t(c) for c in cores], idx, off, nt, mode).cpu().numpy()
    m = module(p, q, r, cores, nt, mode, sparse=False)
    assert_close(m(t(idx), t(off)).detach().cpu().numpy(), ref, f"{mode} forward")
    m2 = module(p, q, r, cores, nt, mode, sparse=False, include_last_offset=False)
    got = m2(t(idx).int(), t(off[:-1]).int())
    assert_close(got.detach().cpu().numpy(), ref, f"{mode} forward (include_last_offset=False, int32)")
    if geom[0] == "t2":  # (the gathered reference rows are tt_matrix_to_full's rows)
        full = ops.tt_matrix_to_full(p, q, [1] + r + [1], [t(c[0:1]) for c in cores], [1, 0, 2, 3])
        rows = tt_rows_torch(p, q, r, [t(c[0]) for c in cores], idx)
        assert_close(rows.cpu().numpy(), full[t(idx)].cpu().numpy(), "gathered rows")


def test_single_table_module_and_readme_toy():
    """TTEmbeddingBag (forward -> [B, D]) with D = 3, the README's toy shape, in both modes"""
    import tt_embeddings_ops as ops

    p, q, r = [2, 5], [1, 3], [2]
    cores = G.make_cores(3, 1, p, q, r, "signed")
    idx, off = batch(9, 1, 6, 10, long_bag=40)
    for mode in ("mean", "max"):
        m = ops.TTEmbeddingBag(10, 3, r, p, q, use_cache=False, sparse=False, weight_dist="uniform", device=DEV, mode=mode)
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, cores):
                dst.copy_(t(src))
        out = m(t(idx), t(off))
        assert out.shape == (6, 3)
        ref = ref_lookup(p, q, r, [t(c) for c in cores], idx, off, 1, mode)[0]
        assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), f"toy {mode}")


# ---------------------------------------------------------------------------------------------------- module: gradients
def ref_grads(p, q, r, cores_np, idx, off, nt, mode, d_out):
    leaves = [t(c).clone().requires_grad_(True) for c in cores_np]
    ref = ref_lookup(p, q, r, leaves, idx, off, nt, mode)
    ref.backward(t(d_out))
    return ref.detach(), [c.grad.cpu().numpy() for c in leaves]


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("mode,route", MODE_ROUTES, ids=[f"{m}-{r}" for m, r in MODE_ROUTES])
def test_dense_core_gradients_match_torch_autograd(geom, mode, route, monkeypatch):
    use_route(route, monkeypatch)
    _, p, q, r = geom
    nt, B, E_ = 3, 13, int(np.prod(p))
    cores = G.make_cores(31, nt, p, q, r, "signed")
    idx, off = batch(6, nt, B, E_, long_bag=60)
    d_out = G.make_grad(7, nt, B, int(np.prod(q)))
    ref, grads = ref_grads(p, q, r, cores, idx, off, nt, mode, d_out)
    m = module(p, q, r, cores, nt, mode, sparse=False)
    out = m(t(idx), t(off))
    assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), f"{mode} forward")
    out.backward(t(d_out))
    for k in range(len(p)):
        assert_close(m.tt_cores[k].grad.cpu().numpy(), grads[k], f"{mode} grad{k}")


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("mode", ["mean", "max"])
@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_fused_optimizer_steps_track_the_gradients(geom, mode, optim):
    """three fused steps on changing batches: after each, the cores (and Adagrad's state) are the update of the cores
    before the step along torch's gradient at those cores"""
    import tt_embeddings_ops as ops

    _, p, q, r = geom
    nt, B, E_, D = 2, 11, int(np.prod(p)), int(np.prod(q))
    cores = G.make_cores(41, nt, p, q, r, "signed")
    opt = ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD
    m = module(p, q, r, cores, nt, mode, sparse=True, optimizer=opt, learning_rate=LR, eps=EPS)
    for step in range(3):
        idx, off = batch(50 + step, nt, B, E_, long_bag=40)
        d_out = G.make_grad(60 + step, nt, B, D)
        before = [c.detach().cpu().numpy().copy() for c in m.tt_cores]
        state0 = [s.cpu().numpy().copy() for s in m.optimizer_state] if optim == "adagrad" else None
        _, grads = ref_grads(p, q, r, before, idx, off, nt, mode, d_out)
        m(t(idx), t(off)).backward(t(d_out))
        for k in range(len(p)):
            got = m.tt_cores[k].detach().cpu().numpy()
            if optim == "sgd":
                assert_close(got, before[k] - np.float32(LR) * grads[k], f"step {step} sgd core{k}")
            else:
                s = state0[k] + grads[k] * grads[k]
                assert_close(m.optimizer_state[k].cpu().numpy(), s, f"step {step} adagrad state{k}")
                ref_w = before[k] - np.float32(LR) * grads[k] / (np.sqrt(s) + np.float32(EPS))
                assert_adagrad_close(got, ref_w, grads[k], f"step {step} adagrad core{k}", state0=state0[k])


@pytest.mark.parametrize("first", [0, 1])
def test_max_tie_between_different_indices_goes_to_the_earlier_lookup(first):
    """two core-0 slices made equal: indices that differ only there have identical rows; in a bag holding both, every
    column is a tie and the whole gradient goes to the earlier lookup's slice"""
    p, q, r = [6, 5, 7], [4, 4, 4], [16, 16]
    cores = G.make_cores(71, 1, p, q, r, "signed")
    cores[0][0, 4] = cores[0][0, 1]
    a, b = 1 * 35 + 2 * 7 + 3, 4 * 35 + 2 * 7 + 3  # (i0 = 1 / 4, same i1, i2)
    pair = [a, b] if first == 0 else [b, a]
    idx = np.array(pair + [0 * 35 + 1], np.int64)  # bag 0: the tied pair; bag 1: another row
    off = np.array([0, 2, 3], np.int64)
    m = module(p, q, r, cores, 1, "max", sparse=False)
    out = m(t(idx), t(off))
    rows = tt_rows_torch(p, q, r, [t(c[0]) for c in cores], idx[:2]).cpu().numpy()
    assert np.array_equal(rows[0], rows[1])
    out.backward(torch.ones_like(out))
    g0 = m.tt_cores[0].grad[0].cpu().numpy()
    winner, loser = pair[0] // 35, pair[1] // 35
    assert np.abs(g0[winner]).max() > 0
    assert (g0[loser] == 0).all(), "the later lookup of a tie must receive no gradient"


# ----------------------------------------------------------------------------------------------------------- mean routes
def test_mean_with_a_live_cache(node):
    """after cache_populate(): the mean output is the sum route's output over the bag lengths (and torch's mean), one fused SGD
    step moves each cached lookup's cache row by -lr * (bag gradient / bag length), and the cores as the sum route does with
    the gradient divided by the bag lengths"""
    import tt_embeddings_ops as ops

    p, q, r = [20, 22, 25], [4, 4, 4], [16, 16]
    E_, D = int(np.prod(p)), 64
    cores = G.make_cores(81, 1, p, q, r, "signed")
    rs = np.random.RandomState(82)
    # the warm-up batch holds 100 distinct keys, all of which fit in the 128 cache rows: populate evicts nothing, so the hash
    # table's layout (which concurrent inserts leave to arrival order) cannot move a cached key.  The step's batch mixes those
    # keys (hits) with keys never counted (misses, contracted).
    warm_idx, warm_off = np.arange(100, dtype=np.int64), np.array([0, 50, 100], np.int64)
    idx, off = batch(83, 1, 64, 100, long_bag=50)
    idx = np.where(rs.rand(idx.size) < 0.5, idx, rs.randint(5000, E_, size=idx.size)).astype(np.int64)
    d_out = rs.standard_normal((64, D)).astype(np.float32)
    cnt = np.maximum(np.diff(off), 1).astype(np.float32)
    mods = {}
    for mode in ("sum", "mean"):
        m = ops.TTEmbeddingBag(E_, D, r, p, q, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, use_cache=True,
                               cache_size=128, hashtbl_size=1024, weight_dist="uniform", device=DEV, mode=mode,
                               deterministic_cache_update=True)
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, cores):
                dst.copy_(t(src))
        with torch.no_grad():
            m(t(warm_idx), t(warm_off))  # (counts the warm-up keys)
        m.cache_populate()
        mods[mode] = m
    cw0 = mods["mean"].cache_weight.detach().cpu().numpy().copy()
    outs = {}
    for mode, d in (("sum", d_out / cnt[:, None]), ("mean", d_out)):  # (each module's step, forward then backward)
        out = mods[mode](t(idx), t(off))
        outs[mode] = out.detach().cpu().numpy()
        out.backward(t(d))
    assert_close(outs["mean"], outs["sum"] / cnt[:, None], "cache-live mean forward")
    ref = ref_lookup(p, q, r, [t(c) for c in cores], idx, off, 1, "mean")[0]
    assert_close(outs["mean"], ref.cpu().numpy(), "cache-live mean vs torch")
    # the cached lookups' update, from the hash table: cache row loc(key) -= lr * (bag gradient / bag length)
    m = mods["mean"]
    ht, cs = m.hashtbl.cpu().numpy(), m.cache_state.cpu().numpy()
    loc = {int(ht[s]): int(cs[s]) for s in range(ht.size) if ht[s] >= 0 and cs[s] >= 0}
    want = cw0.astype(np.float64)
    hits = 0
    for b in range(off.size - 1):
        for n in range(int(off[b]), int(off[b + 1])):
            if int(idx[n]) in loc:
                want[loc[int(idx[n])]] -= LR * d_out[b].astype(np.float64) / cnt[b]
                hits += 1
    assert 0 < hits < idx.size, "the batch must mix cached and contracted lookups"
    cw = m.cache_weight.detach().cpu().numpy()
    assert_close(cw, want, "cache_weight after one step")
    for k in range(3):  # (the contracted lookups: the cores move as the sum route's do with the gradient / bag length)
        assert_close(mods["mean"].tt_cores[k].detach().cpu().numpy(), mods["sum"].tt_cores[k].detach().cpu().numpy(),
                     f"core{k} after one step")


def test_mean_with_a_device_side_lookup_count(node):
    """forward(n_dev=): a fixed-capacity index buffer, the first n live -- the same output and gradients as the plain call"""
    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B, D = 2, 16, 64
    cores = G.make_cores(91, nt, p, q, r, "signed")
    idx, off = batch(92, nt, B, int(np.prod(p)), long_bag=30)
    n = idx.size
    padded = np.concatenate([idx, np.random.RandomState(93).randint(0, int(np.prod(p)), size=100)]).astype(np.int64)
    d_out = G.make_grad(94, nt, B, D)
    ma = module(p, q, r, cores, nt, "mean", sparse=False)
    mb = module(p, q, r, cores, nt, "mean", sparse=False)
    oa = ma(t(idx), t(off))
    ob = mb(t(padded), t(off), n_dev=torch.tensor([n], dtype=torch.int32, device=DEV))
    assert_close(ob.detach().cpu().numpy(), oa.detach().cpu().numpy(), "mean forward(n_dev=)")
    oa.backward(t(d_out))
    ob.backward(t(d_out))
    for k in range(3):
        assert_close(mb.tt_cores[k].grad.cpu().numpy(), ma.tt_cores[k].grad.cpu().numpy(), f"mean n_dev grad{k}")


# ------------------------------------------------------------------------------------------------ capture, determinism
@pytest.mark.parametrize("mode", ["mean", "max"])
def test_captured_step_replays_bit_identically_to_eager_steps(mode):
    import tt_embeddings_ops as ops
    import ttx_graph

    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B = 2, 64
    cores = G.make_cores(101, nt, p, q, r, "signed")
    idx, off = batch(102, nt, B, int(np.prod(p)), long_bag=40)
    g = t(G.make_grad(103, nt, B, 64))

    def run(graphed):
        m = module(p, q, r, cores, nt, mode, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR)
        step = lambda i, o, d: m(i, o).backward(d)  # noqa: E731
        if graphed:
            gs = ttx_graph.GraphedStep(step, (t(idx), t(off), g), warmup=2)
            for _ in range(3):
                gs(t(idx), t(off), g)
        else:
            for _ in range(5):
                step(t(idx), t(off), g)
        torch.cuda.synchronize()
        return [c.detach().clone() for c in m.tt_cores]

    eager, replayed = run(False), run(True)
    for k in range(3):
        assert torch.equal(eager[k], replayed[k]), f"{mode}: core {k} differs between replay and eager"


def test_max_mode_adagrad_is_bit_deterministic():
    import tt_embeddings_ops as ops

    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B = 3, 256
    cores = G.make_cores(111, nt, p, q, r, "signed")
    runs = []
    for _ in range(2):
        m = module(p, q, r, cores, nt, "max", sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=LR, eps=EPS)
        for s in range(3):
            idx, off = batch(112 + s, nt, B, 3000, long_bag=100)  # (a small key space: slices shared by many lookups)
            m(t(idx), t(off)).backward(t(G.make_grad(120 + s, nt, B, 64)))
        torch.cuda.synchronize()
        runs.append([c.detach().clone() for c in m.tt_cores] + [s_.clone() for s_ in m.optimizer_state])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_mode_sum_is_the_default_bit_for_bit(node):
    import tt_embeddings_ops as ops

    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B = 2, 32
    cores = G.make_cores(131, nt, p, q, r, "signed")
    idx, off = batch(132, nt, B, int(np.prod(p)), long_bag=20)
    d = t(G.make_grad(133, nt, B, 64))
    res = []
    for kw in ({}, {"mode": "sum"}):
        m = ops.TableBatchedTTEmbeddingBag(nt, int(np.prod(p)), 64, r, p, q, use_cache=False, weight_dist="uniform", device=DEV,
                                           sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, **kw)
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, cores):
                dst.copy_(t(src))
        out = m(t(idx), t(off))
        out.backward(d)
        res.append([out.detach().clone()] + [c.detach().clone() for c in m.tt_cores])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    import tt_embeddings_ops as ops

    p, q, r = [5, 8], [3, 4], [6]
    cores = G.make_cores(141, 1, p, q, r)
    idx, off = batch(142, 1, 4, 40, long_bag=3)
    for mode in ("mean", "max"):
        m = module(p, q, r, cores, 1, mode, sparse=False)
        with pytest.raises(ValueError):
            m(t(idx), t(off), per_sample_weights=torch.ones(idx.size, device=DEV))
    with pytest.raises(NotImplementedError):
        ops.TTEmbeddingBag(40, 12, r, p, q, use_cache=True, cache_size=4, hashtbl_size=16, device=DEV, mode="max")
    with pytest.raises(NotImplementedError):
        module(p, q, r, cores, 1, "max", dedup=True)
    m = module(p, q, r, cores, 1, "max", sparse=False)
    with pytest.raises(NotImplementedError):
        m(t(idx), t(off), n_dev=torch.tensor([idx.size], dtype=torch.int32, device=DEV))
