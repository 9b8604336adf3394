"""The hot row table of TTInferenceBag without a GPU: the torch-op path against a float64 reference -- a hit is the
stored hot row widened exactly, a miss the float64 chain product on the bf16 cores -- within the derived bound of tests/bf16_ref.py;
the buffers; the refusals; the argument errors of the two C entry points; the compiler's resource report.  `hot_set`, `mixed_batch`
and `hot_reference` are shared with tests/test_infer_hot_gpu.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

import bf16_ref as R
from test_bf16_infer_cpu import _module, ops  # noqa: F401  (`ops`: the fixture that puts the modules on the CPU oracle engine)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hot_set(rs, tables, E, K):
    """K distinct keys as one index array per table, in random order: the smallest and the largest key of the key space and row 5 of
    table 0 among them (K = 1: the largest alone); row 5 of table 1 never"""
    forced = [tables * E - 1] if K == 1 else [0, tables * E - 1, 5]
    pool = [k for k in rs.permutation(tables * E) if k not in forced and k != E + 5][:K - len(forced)]
    keys = rs.permutation(np.array(forced + pool, dtype=np.int64))
    return [keys[keys // E == t] - t * E for t in range(tables)]


def mixed_batch(rs, hot, E):
    """6 bags per table: empty, hits only, misses only, 152 slots of both (a second and a third probe round), two short random ones"""
    bags = []
    for h in hot:
        cold = np.setdiff1d(np.arange(E), h)
        both = np.concatenate([rs.choice(h, 75) if h.size else cold[:0], rs.choice(cold, 75), [0, E - 1]])
        bags += [cold[:0], rs.choice(h, 7) if h.size else cold[:0], rs.choice(cold, 9), rs.permutation(both),
                 rs.randint(0, E, size=rs.randint(0, 6)), rs.randint(0, E, size=rs.randint(0, 6))]
    return np.concatenate(bags).astype(np.int64), np.concatenate([[0], np.cumsum([b.size for b in bags])]).astype(np.int64)


def hot_reference(inf, cores, p, q, r, idx, off, tables):
    """-> (pooled float64 reference, its bound, the hit flags): miss rows with their row bound, hit rows exact with bound 0"""
    E, nb = inf.num_embeddings, len(off) - 1
    keys, hrows = inf.hot_keys.cpu().numpy(), inf.hot_rows.float().cpu().numpy().astype(np.float64)
    key = np.repeat(np.arange(nb) // (nb // tables), np.diff(off)) * E + idx
    uk, inv = np.unique(key, return_inverse=True)  # (a row per distinct key: the large batch repeats its keys)
    rows, bnd = (a[inv] for a in R.rows64(*R.slices(cores, p, q, r, uk % E, uk // E)))
    pos = np.minimum(np.searchsorted(keys, key), len(keys) - 1)
    hit = keys[pos] == key
    rows[hit], bnd[hit] = hrows[pos[hit]], 0.0
    return R.pool64(rows, bnd, off, mean=inf.mode == "mean") + (hit,)


@pytest.mark.parametrize("q,r,tables,mode,K", [([4, 4, 4], [32, 32], 3, "mean", 37), ([3, 4, 5], [13, 12], 1, "sum", 1)])
def test_torch_path_meets_the_bound(ops, q, r, tables, mode, K):  # noqa: F811
    import ttx_infer

    F, p = ttx_infer.TTInferenceBag.from_module, [5, 6, 7]
    m, E, D = _module(ops, "batched", tables, q, r, mode=mode)
    rs = np.random.RandomState(5)
    hot = hot_set(rs, tables, E, K)
    inf = F(m, hot_indices=[torch.from_numpy(np.concatenate([h, h[:1]])) for h in hot])  # (unsorted, one duplicate each)
    assert inf.hot_rows_count == K and tuple(inf.hot_rows.shape) == (K, D) and inf.hot_rows.dtype == torch.bfloat16
    assert not list(inf.parameters()) and {"hot_keys", "hot_rows"} <= set(inf.state_dict()) and "hot_keys" not in F(m).state_dict()
    # sorted, deduplicated, key = table * num_embeddings + index; the rows are the module's own, rounded once
    assert np.array_equal(inf.hot_keys.numpy(), np.sort(np.concatenate([h + t * E for t, h in enumerate(hot)])))
    assert torch.equal(inf.hot_rows, F(m)._rows_torch(inf.hot_keys % E, inf.hot_keys // E).to(torch.bfloat16))
    idx, off = mixed_batch(rs, hot, E)
    out = inf(torch.from_numpy(idx), torch.from_numpy(off))
    ref, bnd, hit = hot_reference(inf, [R.to_bf16(c.detach().numpy()) for c in m.tt_cores], p, q, r, idx, off, tables)
    err = np.abs(out.numpy().astype(np.float64).reshape(ref.shape) - ref)
    assert hit.any() and not hit.all() and (err <= bnd).all(), float(np.max(err / np.maximum(bnd, 1e-300)))
    assert torch.equal(out, inf(torch.from_numpy(idx).int(), torch.from_numpy(off).int()))
    other = F(m, hot_indices=[torch.arange(h.size) for h in hot])  # state_dict round trip into a module with another hot set
    other.load_state_dict(inf.state_dict())
    assert torch.equal(other(torch.from_numpy(idx), torch.from_numpy(off)), out)


def test_refusals_the_disabled_case_and_a_live_cache(ops):  # noqa: F811
    import ttx_infer

    F, q, r = ttx_infer.TTInferenceBag.from_module, [2, 2, 4], [16, 16]
    m, E, D = _module(ops, "batched", 2, q, r)
    for bad in (torch.tensor([E]), torch.tensor([-1]), torch.tensor([[1]]), torch.tensor([1.0])):
        with pytest.raises(ValueError, match="hot_indices"):
            F(m, hot_indices=[bad, torch.tensor([0])])
    for kw, why in ((dict(hot_indices=torch.tensor([0])), "per table"), (dict(hot_from_cache=True), "live")):
        with pytest.raises(ValueError, match=why):
            F(m, **kw)
    with pytest.raises(ValueError, match="fp32"):
        F(ops.TableBatchedTTEmbeddingBag(1, 210, 8, [128, 128], [5, 6, 7], [2, 2, 2], weight_dist="uniform", device="cpu"),
          hot_indices=torch.tensor([3]))
    idx, off = torch.arange(12) % E, torch.tensor([0, 3, 6, 9, 12])
    for none in (None, [torch.zeros(0, dtype=torch.int64)] * 2):
        inf = F(m, hot_indices=none)
        assert inf.hot_rows_count == 0 and len(list(inf.buffers())) == 3 and torch.equal(inf(idx, off), F(m)(idx, off))
    # a one-table source whose cache went live: refused without the flag, word for word as before; with it, its rows are served
    c, E, D = _module(ops, "bag", 1, q, r, use_cache=True, cache_size=8, hashtbl_size=64)
    c.hashtbl[3], c.cache_state[3], c.hashtbl[9], c.cache_state[9], c.warmup = 17, 1, 4, 0, False
    with torch.no_grad():
        c.cache_weight.copy_(torch.randn(8, D))
    with pytest.raises(ValueError, match=r"cache_populate\(write_back"):
        F(c)
    with pytest.raises(ValueError, match="not both"):
        F(c, hot_indices=torch.tensor([1]), hot_from_cache=True)
    inf = F(c, hot_from_cache=True)
    assert inf.hot_keys.tolist() == [4, 17]
    assert torch.equal(inf(torch.tensor([17, 4]), torch.tensor([0, 1, 2])), c.cache_weight.detach()[[1, 0]].to(torch.bfloat16).float())


def test_argument_errors_return_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced; without a GPU a call that reached the runtime would return -4)"""
    i32, i64, vp, fake, odd = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, 4096, 4100
    for name in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", name))
        lib.ttx_last_error.restype = ctypes.c_char_p
        lib.ttx_hot_probe_pool.argtypes = [i32, i64, i32, i64, vp, vp, i64, i64, vp, vp, vp, vp, vp]
        lib.ttx_bag_sum_pool_add.argtypes = [i64, i32, vp, vp, vp, vp, vp]

        def probe(**kw):  # (num_tables, B, D, nnz, indices, offsets, key_stride, K, hot_keys, hot_rows, masked_indices, hit_sum)
            a = dict(dict(T=2, B=4, D=64, nnz=100, idx=fake, off=fake, stride=1000, K=5, keys=fake, rows=fake, masked=fake, hit=fake), **kw)
            return lib.ttx_hot_probe_pool(*a.values(), None)

        for kw in (dict(T=0), dict(B=-1), dict(D=0), dict(nnz=-1), dict(nnz=1 << 31), dict(K=-1), dict(K=1 << 31), dict(stride=0),
                   dict(stride=1 << 62), dict(idx=None), dict(off=None), dict(masked=None), dict(hit=None), dict(keys=None),
                   dict(rows=None), dict(idx=odd), dict(keys=odd), dict(hit=fake + 2), dict(rows=fake + 1)):
            assert probe(**kw) == -1 and b"hot_probe_pool" in lib.ttx_last_error(), kw
        assert probe(nnz=0, idx=None, masked=None) == 0 and probe(B=0, off=None, hit=None) == 0  # nothing launched

        def pool(**kw):  # (nb, D, offsets, rows, addend, output)
            return lib.ttx_bag_sum_pool_add(*dict(dict(nb=4, D=8, off=fake, rows=fake, add=fake, out=fake), **kw).values(), None)

        for kw in (dict(nb=-1), dict(nb=1 << 31), dict(D=0), dict(off=None), dict(rows=None), dict(add=None), dict(out=None),
                   dict(off=odd), dict(rows=fake + 2), dict(add=fake + 1)):
            assert pool(**kw) == -1 and b"bag_sum_pool_add" in lib.ttx_last_error(), kw
        assert pool(nb=0, off=None, rows=None, add=None, out=None) == 0


def test_hot_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950; the figures are in DESIGN.md 4.23"""
    from test_kernel_resources import resources

    res = resources("ttx_hot.hip")
    assert [sum(w in k for k in res) for w in ("hot_probe_pool_kernel", "bag_sum_pool_add_kernel")] == [2, 2] and len(res) == 4, list(res)
    assert all(v["ScratchSize"] == 0 and v["Occupancy"] >= 6 for v in res.values()), res
