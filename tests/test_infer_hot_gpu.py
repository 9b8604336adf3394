"""GPU tests of TTInferenceBag's hot row table (include/ttx.h "hot rows of the inference forward").

The module output against the float64 reference of tests/test_infer_hot_cpu.py: a hit row is the stored hot row widened exactly
(bound 0), a miss row the float64 chain product on the bf16 cores (its row bound, tests/bf16_ref.py), a bag the float64 sum with
len 2^-24 sum |row| for pooling and one rounding for the mean.  The bound is derived: there is no tolerance to tune.  K = 1 keeps
the largest key alone; every larger K the smallest and the largest key and a row that is hot in table 0 and cold in table 1."""
import functools

import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G
from test_infer_hot_cpu import hot_reference, hot_set, mixed_batch

pytestmark = pytest.mark.gpu

P = [16, 18, 20]  # 5,760 rows a table: room for 4,096 hot keys
E = int(np.prod(P))
# a shape per route whose kernels differ, D = 64, and D % 8 != 0 (D = 60: the scalar row path of the probe)
GEOMS = {"bf16": ([4, 4, 4], [32, 32], {}), "bf16m": ([2, 2, 16], [16, 16], dict(mfma_tail=True)), "scalar": ([3, 4, 5], [13, 12], {})}


def t(a):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _source(geom, kind, tables, mode):
    """-> (module on the GPU, its cores rounded to bf16 as numpy): built once per shape, never changed"""
    import tt_embeddings_ops as ops

    q, r, _ = GEOMS[geom]
    D, kw = int(np.prod(q)), dict(weight_dist="uniform", device="cuda:0")
    if kind == "embedding":
        m = ops.TTEmbedding(E, D, list(r), P, list(q), **kw)
    elif kind == "bag":
        m = ops.TTEmbeddingBag(E, D, list(r), P, list(q), mode=mode, use_cache=False, **kw)
    else:
        m = ops.TableBatchedTTEmbeddingBag(tables, E, D, list(r), P, list(q), mode=mode, **kw)
    cores = G.make_cores(81, tables, P, q, r, "signed")
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(t(src))
    return m, [R.to_bf16(c) for c in cores]


def _frozen(geom, kind, tables, mode, K):
    import ttx_infer

    m, cores = _source(geom, kind, tables, mode)
    rs = np.random.RandomState(82)
    hot = hot_set(rs, tables, E, K)
    given = [t(h) for h in hot]
    inf = ttx_infer.TTInferenceBag.from_module(m, hot_indices=given[0] if kind != "batched" else given, **GEOMS[geom][2])
    assert inf.route == ("bf16" if geom == "scalar" else geom) and inf.hot_rows_count == K and not list(inf.parameters())
    return inf, cores, hot, rs


def _check(inf, cores, geom, idx, off, tables, out):
    ref, bnd, hit = hot_reference(inf, cores, P, *GEOMS[geom][:2], idx, off, tables)
    err = np.abs(out.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
    ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
    print(f"{geom} tables={tables} K={inf.hot_rows_count} {inf.mode}: {int(hit.sum())} of {hit.size} hits, worst err / bound {ratio:.5f}")
    assert (err <= bnd).all(), ratio
    return hit


@pytest.mark.parametrize("K", [1, 37, 4096])
@pytest.mark.parametrize("tables", [1, 3])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_mixed_bags_meet_the_bound(geom, tables, K):
    """per table: an empty bag, a bag of hits only, one of misses only, one of 152 slots (further probe rounds), two short ones;
    sum on one table, mean on three; int32 indices give the same bits"""
    inf, cores, hot, rs = _frozen(geom, "batched", tables, "mean" if tables == 3 else "sum", K)
    idx, off = mixed_batch(rs, hot, E)
    out = inf(t(idx), t(off))
    assert tuple(out.shape) == (tables, 6, inf.embedding_dim) and out.dtype == torch.float32
    hit = _check(inf, cores, geom, idx, off, tables, out)
    assert hit.any() and not hit.all() and torch.equal(out, inf(t(idx).int(), t(off).int()))


@pytest.mark.parametrize("batch", ["all hits", "all misses", "40,000 slots"])
def test_whole_batches(batch):
    """nothing left to contract, nothing found, and a batch above 32,768 slots (the multi-launch compaction)"""
    inf, cores, hot, rs = _frozen("bf16m", "bag", 1, "sum", 37)
    cold = np.setdiff1d(np.arange(E), hot[0])
    if batch == "40,000 slots":
        idx = np.concatenate([rs.choice(hot[0], 15000), rs.choice(cold[:300], 25000)])[rs.permutation(40000)].astype(np.int64)
        off = np.array([0, 1, 20000, 20000, 40000], dtype=np.int64)
    else:
        idx = rs.choice(hot[0] if batch == "all hits" else cold, 300).astype(np.int64)
        off = np.concatenate([[0], np.sort(rs.randint(0, 301, size=7)), [300]]).astype(np.int64)
    hit = _check(inf, cores, "bf16m", idx, off, 1, inf(t(idx), t(off)))
    assert hit.all() if batch == "all hits" else (not hit.any() if batch == "all misses" else hit.any())


def test_embedding_source_serves_positions_as_bags_of_one_slot():
    inf, cores, hot, rs = _frozen("bf16", "embedding", 1, "sum", 37)
    idx = np.concatenate([rs.choice(hot[0], 20), rs.randint(0, E, size=25)])[rs.permutation(45)].reshape(5, 9).astype(np.int64)
    out = inf(t(idx))
    assert tuple(out.shape) == (5, 9, 64)
    hit = _check(inf, cores, "bf16", idx.reshape(-1), np.arange(46, dtype=np.int64), 1, out)
    rows = inf.hot_rows.float()[torch.searchsorted(inf.hot_keys, t(idx.reshape(-1)[hit]))]
    assert torch.equal(out.view(-1, 64)[t(hit)], rows)  # a hit position IS its stored row


def test_captured_replays_equal_eager_and_no_hot_set_changes_no_bit():
    import ttx_infer

    inf, cores, hot, rs = _frozen("bf16", "batched", 3, "mean", 37)
    ti, to = (t(a) for a in mixed_batch(rs, hot, E))
    out = inf(ti, to)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture's stream (its workspace)
        inf(ti, to)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        g_out = inf(ti, to)
    for k in range(2):
        g_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, out), f"replay {k}"
    m = _source("bf16", "batched", 3, "mean")[0]
    for none in (None, [torch.zeros(0, dtype=torch.int64)] * 3):  # no hot set: the buffers and the bits of the module without the argument
        plain = ttx_infer.TTInferenceBag.from_module(m, hot_indices=none)
        assert plain.hot_rows_count == 0 and len(list(plain.buffers())) == 3
        assert torch.equal(plain(ti, to), ttx_infer.TTInferenceBag.from_module(m)(ti, to))


@pytest.mark.parametrize("tables", [1, 3])
def test_hot_from_cache_serves_the_trained_cache_rows(tables):
    """a cached module gone live: refused without the flag as before; with it every cached key returns its cache_weight row rounded
    to bf16, exactly, and a mixed batch meets the bound"""
    import tt_embeddings_ops as ops
    import ttx_infer

    q, r, _ = GEOMS["bf16"]
    kw = dict(weight_dist="uniform", device="cuda:0", use_cache=True, cache_size=48, hashtbl_size=1024)
    m = ops.TTEmbeddingBag(E, 64, r, P, q, **kw) if tables == 1 else ops.TableBatchedTTEmbeddingBag(tables, E, 64, r, P, q, **kw)
    rs = np.random.RandomState(84)
    m(t(rs.randint(0, 200, size=tables * 400).astype(np.int64)), t(np.arange(0, tables * 400 + 1, 40, dtype=np.int64)))  # (counted)
    m.cache_populate()
    with torch.no_grad():
        m.cache_weight.add_(t(rs.standard_normal(tuple(m.cache_weight.shape)).astype(np.float32)))  # trained away from the cores
    with pytest.raises(ValueError, match=r"cache_populate\(write_back"):
        ttx_infer.TTInferenceBag.from_module(m)
    inf = ttx_infer.TTInferenceBag.from_module(m, hot_from_cache=True)
    state, tbl = m.cache_state.cpu().numpy(), m.hashtbl.cpu().numpy()
    slots = np.nonzero(state >= 0)[0]
    keys, n = tbl[slots], len(slots)  # (prod(P) == E: the source's keys are the module's)
    assert inf.hot_rows_count == n > 8 and np.array_equal(inf.hot_keys.cpu().numpy(), np.sort(keys))
    want = m.cache_weight.detach()[t(state[slots].astype(np.int64))].to(torch.bfloat16).float()
    lens = np.zeros((tables, n), dtype=np.int64)  # bag (table, j) holds key j where it is that table's
    lens[keys // E, np.arange(n)] = 1
    out = inf(t((keys % E)[np.argsort(keys // E, kind="stable")]), t(np.concatenate([[0], np.cumsum(lens.reshape(-1))])))
    assert torch.equal(out.view(tables, n, 64)[t(keys // E), torch.arange(n)], want)
    idx, off = mixed_batch(rs, [np.sort(keys[keys // E == k] % E) for k in range(tables)], E)
    hit = _check(inf, [R.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores], "bf16", idx, off, tables, inf(t(idx), t(off)))
    assert hit.any() and not hit.all()
