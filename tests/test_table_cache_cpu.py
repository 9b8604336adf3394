"""CPU tests (no GPU) of the row cache over several tables, `TableBatchedTTEmbeddingBag(num_tables > 1, use_cache=True)`: the C ABI
of ttx_table_keys / ttx_table_keys_split / ttx_cache_populate_t (declared, exported by both libraries, argument checks with
pointers that are never dereferenced), the shim's calls, the compiler's resource report of csrc/ttx_cache_tables.hip, and -- on
top of the oracle engine -- what the module accepts, counts and refuses."""
import collections
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import oracle_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R = [5, 6, 7], [2, 2, 3], [4, 3]
E_, D_, STRIDE = 200, 12, 5 * 6 * 7  # (num_embeddings below prod(p): the key stride is prod(p), not num_embeddings)
NT, B = 3, 4


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


def bags(ops, num_tables=NT, **kw):
    kw.setdefault("sparse", False)
    torch.manual_seed(3)
    return ops.TableBatchedTTEmbeddingBag(num_tables, E_, D_, R, P, Q, weight_dist="uniform", device="cpu", **kw)


def batch(seed, empty_table=None):
    """NT * B bags of 0 .. 4 lookups, table-major; bag 1 of table 0 is empty, `empty_table` has no lookups at all"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(0, 5, size=NT * B)
    lens[1] = 0
    if empty_table is not None:
        lens[empty_table * B:(empty_table + 1) * B] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rs.randint(0, 20, size=int(off[-1])).astype(np.int64)  # (a small range: the same local index turns up in every table)
    table = np.repeat(np.arange(NT * B) // B, lens)
    return idx, off, idx + table * STRIDE


# ----------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_and_exported_and_check_their_arguments():
    text = open(os.path.join(ROOT, "include", "ttx.h")).read()
    assert "row cache over several tables (not in the reference)" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ttx_table_keys\s*\(\s*int64_t nnz,\s*const int64_t\*\s*indices,\s*int32_t num_tables,\s*int64_t B,"
                     r"\s*const int64_t\*\s*offsets,\s*int64_t key_stride,\s*int64_t\*\s*keys,\s*int64_t H,\s*int64_t\*\s*upd_hashtbl,"
                     r"\s*int64_t\*\s*upd_cache_freq,\s*ttx_stream_t stream\)", hdr), "ttx_table_keys is not declared"
    assert re.search(r"\bint\s+ttx_table_keys_split\s*\(\s*int64_t n,\s*const int32_t\*\s*n_dev,\s*int32_t num_tables,\s*int64_t B,"
                     r"\s*int64_t key_stride,\s*const int64_t\*\s*keys,\s*const int64_t\*\s*bagrow,\s*int64_t\*\s*out_indices,"
                     r"\s*int64_t\*\s*out_tableidx,\s*int64_t\*\s*out_rowidx,\s*ttx_stream_t stream\)", hdr), "ttx_table_keys_split"
    assert re.search(r"\bint\s+ttx_cache_populate_t\s*\(\s*const ttx_geom\*\s*g,", hdr), "ttx_cache_populate_t is not declared"
    assert re.search(r"\bsize_t\s+ttx_cache_populate_t_workspace_bytes\s*\(", hdr)
    i64, i32, vp, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
    fake, odd4, odd2 = vp(4096), vp(4100), vp(4098)  # (never dereferenced: every call below returns before a launch)
    import tt_embeddings as E

    geom = E._geom(NT, P, Q, [1] + R + [1])
    mixed = E._geom(NT, [P, P, P], Q, [1] + R + [1])
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        keys, split, pop = lib.ttx_table_keys, lib.ttx_table_keys_split, lib.ttx_cache_populate_t
        #               nnz  idx nt   B    off stride keys H   hashtbl freq stream
        keys.argtypes = [i64, vp, i32, i64, vp, i64, vp, i64, vp, vp, vp]
        #                n    dev nt   B    stride keys bagrow idx tab row stream
        split.argtypes = [i64, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]
        #              g   cores H   ht  freq state cs  D    cw  stride flags ws  bytes stream
        pop.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, vp, i64, i32, vp, sz, vp]
        # nothing to do: 0, and nothing touches a device (no buffers at all)
        assert keys(0, None, NT, B, None, STRIDE, None, 0, None, None, None) == 0
        assert split(0, None, NT, B, STRIDE, None, None, None, None, None, None) == 0
        ok = dict(nnz=8, idx=fake, nt=NT, B=B, off=fake, stride=STRIDE, keys=fake, H=64, ht=fake, freq=fake)
        bad_keys = [dict(nnz=-1), dict(nnz=1 << 31),                                   # negative size, nnz >= 2^31
                    dict(B=0), dict(B=-3), dict(nt=0), dict(nt=-1), dict(stride=0), dict(stride=-5),
                    dict(nt=1 << 20, B=1 << 20),                                        # more than 2^31 bags
                    dict(stride=1 << 61),                                               # num_tables * key_stride >= 2^62
                    dict(idx=None), dict(off=None), dict(keys=None),                    # NULL that would be read / written
                    dict(ht=None), dict(freq=None), dict(H=0), dict(H=1 << 31),         # counting: both tables, H in (0, 2^31)
                    dict(idx=odd4), dict(off=odd4), dict(keys=odd4), dict(ht=odd4), dict(freq=odd4)]  # int64 pointers, 8-byte aligned
        for change in bad_keys:
            a = dict(ok, **change)
            rc = keys(a["nnz"], a["idx"], a["nt"], a["B"], a["off"], a["stride"], a["keys"], a["H"], a["ht"], a["freq"], None)
            assert rc == -1, ("ttx_table_keys", so, change)
            assert b"table_keys" in lib.ttx_last_error(), lib.ttx_last_error()
        # the argument errors come first: a bad size is refused for an empty batch too
        assert keys(0, None, NT, 0, None, STRIDE, None, 0, None, None, None) == -1
        oks = dict(n=8, dev=None, nt=NT, B=B, stride=STRIDE, keys=fake, bagrow=fake, idx=fake, tab=fake, row=fake)
        bad_split = [dict(n=-1), dict(n=1 << 31), dict(B=0), dict(nt=0), dict(stride=0), dict(stride=-1), dict(stride=1 << 61),
                     dict(keys=None), dict(idx=None), dict(tab=None), dict(row=None),   # (row: written when bagrow is given)
                     dict(bagrow=None, idx=None),
                     dict(dev=odd2), dict(keys=odd4), dict(bagrow=odd4), dict(idx=odd4), dict(tab=odd4), dict(row=odd4)]
        for change in bad_split:
            a = dict(oks, **change)
            rc = split(a["n"], a["dev"], a["nt"], a["B"], a["stride"], a["keys"], a["bagrow"], a["idx"], a["tab"], a["row"], None)
            assert rc == -1, ("ttx_table_keys_split", so, change)
            assert b"table_keys_split" in lib.ttx_last_error(), lib.ttx_last_error()
        gp, mp = ctypes.addressof(geom), ctypes.addressof(mixed)
        okp = dict(g=gp, cores=fake, H=64, ht=fake, freq=fake, state=fake, cs=16, D=D_, cw=fake, stride=STRIDE, flags=0, ws=fake,
                   bytes=1 << 30)
        bad_pop = [dict(g=None), dict(g=mp),                                            # no geometry; per-table row factors
                   dict(stride=0), dict(stride=-1), dict(stride=STRIDE + 1), dict(stride=1 << 61),  # key_stride in (0, prod(p)]
                   dict(H=0), dict(H=-1), dict(H=1 << 31), dict(cs=-1), dict(cs=65), dict(D=0), dict(flags=2),
                   dict(cores=None), dict(ht=None), dict(freq=None), dict(state=None), dict(cw=None),
                   dict(ht=odd4), dict(freq=odd4), dict(state=odd2), dict(cw=odd2), dict(ws=odd4)]
        for change in bad_pop:
            a = dict(okp, **change)
            rc = pop(a["g"], a["cores"], a["H"], a["ht"], a["freq"], a["state"], a["cs"], a["D"], a["cw"], a["stride"], a["flags"],
                     a["ws"], a["bytes"], None)
            assert rc == -1, ("ttx_cache_populate_t", so, change)
            assert b"cache_populate_t" in lib.ttx_last_error(), lib.ttx_last_error()
        rc = pop(gp, fake, 64, fake, fake, fake, 16, D_, fake, STRIDE, 0, None, 0, None)  # no workspace: refused before a launch
        assert rc == -2, lib.ttx_last_error()
        lib.ttx_cache_populate_t_workspace_bytes.restype = sz
        lib.ttx_cache_populate_t_workspace_bytes.argtypes = [vp, i64, i64, i32]
        assert lib.ttx_cache_populate_t_workspace_bytes(gp, 64, 16, D_) > 4 * 64 * 8 + 2 * 16 * 8
        assert lib.ttx_cache_populate_t_workspace_bytes(mp, 64, 16, D_) == 0


def test_engine_exposes_the_calls_and_refuses_cpu_tensors():
    import tt_embeddings as E

    assert list(inspect.signature(E.table_keys).parameters) == ["indices", "offsets", "num_tables", "key_stride", "hashtbl", "cache_freq"]
    par = inspect.signature(E.table_keys).parameters
    assert par["hashtbl"].default is None and par["cache_freq"].default is None
    assert list(inspect.signature(E.table_keys_split).parameters) == ["keys", "bagrow", "num_tables", "B", "key_stride", "n_dev"]
    assert inspect.signature(E.table_keys_split).parameters["n_dev"].default is None
    assert callable(E.cache_populate_tables)
    par = inspect.signature(E.cache_forward).parameters
    assert list(par) == ["B", "nnz", "cache_locations", "rowidx", "cache_weight", "output", "skip_dev"] and par["skip_dev"].default is None
    # (nothing existing changed its signature)
    assert list(inspect.signature(E.cache_populate).parameters)[-1] == "reference_exact"
    assert list(inspect.signature(E.update_cache_state).parameters) == ["indices", "hashtbl", "cache_freq"]
    i64 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.table_keys(i64, torch.arange(4), 3, 10)
    with pytest.raises(RuntimeError):
        E.table_keys_split(i64, i64, 3, 1, 10)


def test_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed)"""
    from test_kernel_resources import resources

    res = {k: v for k, v in resources("ttx_cache_tables.hip").items() if "kernel" in k}
    assert len(res) == 2 and all(any(w in k for k in res) for w in ("table_keys_kernel", "table_keys_split_kernel")), sorted(res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 32, (k, r)
        lds = r.get("LDS Size", r.get("LDSSize", 0))
        assert lds == (0 if "split" in k else 8192), (k, r)  # (the staged table boundaries: 1024 int64)


# -------------------------------------------------------------------------------------------------------------- the module
def test_constructor_accepts_several_tables_with_the_one_table_modules_state(ops):
    m = bags(ops, use_cache=True, cache_size=16, hashtbl_size=64, optimizer=ops.OptimType.EXACT_ROWWISE_ADAGRAD, sparse=True)
    one = bags(ops, num_tables=1, use_cache=True, cache_size=16, hashtbl_size=64, optimizer=ops.OptimType.EXACT_ROWWISE_ADAGRAD,
               sparse=True)
    assert list(m.state_dict()) == list(one.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in one.named_parameters()]
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in one.named_buffers()]
    for k, v in m.state_dict().items():  # one cache for all tables: only the cores (and their state) carry a table dimension
        w = one.state_dict()[k]
        assert tuple(v.shape) == tuple(w.shape) or (v.dim() == 3 and v.shape[0] == NT and tuple(v.shape[1:]) == tuple(w.shape[1:])), k
    assert m.warmup and m.use_cache and m.cache_weight.shape == (16, D_) and m.hashtbl.numel() == 64
    assert m._key_stride() == STRIDE


def test_defaults_and_key_space_errors(ops):
    m = bags(ops, use_cache=True)
    assert m.cache_weight.size(0) == int(0.1 * NT * E_) and m.hashtbl.numel() == NT * E_ == m.cache_freq.numel() == m.cache_state.numel()
    one = bags(ops, num_tables=1, use_cache=True)  # (one table: as before)
    assert one.cache_weight.size(0) == int(0.1 * E_) and one.hashtbl.numel() == E_
    with pytest.raises(ValueError, match="hashtbl_size"):
        bags(ops, use_cache=True, cache_size=8, hashtbl_size=1 << 31)
    with pytest.raises(ValueError, match="hashtbl_size"):  # the default, num_tables * num_embeddings, can be too large too
        ops.TableBatchedTTEmbeddingBag(2, 1 << 30, 8, [2, 2], [1 << 10, 1 << 10, 1 << 10], [2, 2, 2], use_cache=True, cache_size=8,
                                       weight_dist="uniform", device="cpu")
    with pytest.raises(ValueError, match="key space"):
        ops.TableBatchedTTEmbeddingBag(4, 1 << 60, 8, [1, 1, 1], [1 << 15] * 4, [2, 2, 2, 1], use_cache=True, cache_size=8,
                                       hashtbl_size=64, weight_dist="uniform", device="cpu")
    with pytest.raises(NotImplementedError):  # unchanged: max pools no cache rows
        bags(ops, use_cache=True, mode="max")


def freq_map(m):
    ht, fr = m.hashtbl.numpy(), m.cache_freq.numpy()
    return {int(k): int(v) for k, v in zip(ht[ht >= 0], fr[ht >= 0])}


def test_cpu_warm_up_counts_keys(ops):
    """two batches -- one with a table that has no lookups -- on a table of 4096 slots for at most 60 distinct keys (the oracle's
    insert drops a key after three probes: asserted not to happen)"""
    m = bags(ops, use_cache=True, cache_size=16, hashtbl_size=4096)
    want = collections.Counter()
    n = 0
    for seed, empty in ((5, None), (6, 1)):
        idx, off, keys = batch(seed, empty)
        out = m(torch.from_numpy(idx), torch.from_numpy(off))
        assert out.shape == (NT, B, D_)
        want.update(keys.tolist())
        n += idx.size
    got = freq_map(m)
    assert sum(got.values()) == n, "a key ran out of probes"
    assert got == dict(want)
    assert any(k >= STRIDE for k in got) and any(k >= 2 * STRIDE for k in got), "keys of tables 1 and 2"
    # the same local index under several tables is several keys
    local = collections.defaultdict(set)
    for k in got:
        local[k % STRIDE].add(k // STRIDE)
    assert any(len(v) == NT for v in local.values())
    assert m.warmup
    # update_cache(indices, offsets) counts keys too, and needs the offsets
    idx, off, keys = batch(7)
    m.update_cache(torch.from_numpy(idx), torch.from_numpy(off))
    want.update(keys.tolist())
    assert freq_map(m) == dict(want)
    with pytest.raises(ValueError, match="offsets"):
        m.update_cache(torch.from_numpy(idx))
    # the forward equals the uncached module's: counting changes nothing else
    twin = bags(ops)
    with torch.no_grad():
        for dst, src in zip(twin.tt_cores, m.tt_cores):
            dst.copy_(src)
    a = m(torch.from_numpy(idx), torch.from_numpy(off))
    b = twin(torch.from_numpy(idx), torch.from_numpy(off))
    assert torch.equal(a, b)


def test_prefetch_is_declined(ops):
    m = bags(ops, use_cache=True, cache_size=16, hashtbl_size=64)
    idx, off, _ = batch(8)
    i, o = torch.from_numpy(idx), torch.from_numpy(off)
    assert m.prefetch(i, o) is False and m.prefetch_many([(i, o), (i, o)]) is False
    m.warmup = False
    assert m.prefetch(i, o) is False and m.prefetch_many([(i, o), (i, o)]) is False
    assert not getattr(m, "_prefetched", None)


def test_what_the_live_cache_over_several_tables_refuses(ops):
    m = bags(ops, use_cache=True, cache_size=16, hashtbl_size=64)
    idx, off, _ = batch(9)
    i, o = torch.from_numpy(idx), torch.from_numpy(off)
    with pytest.raises(NotImplementedError, match="write_back"):
        m.cache_populate(write_back=0.1)
    with pytest.raises(NotImplementedError):  # the oracle's populate decodes one table: nothing goes live on the CPU
        m.cache_populate()
    assert m.warmup
    m.warmup = False  # (as if it had)
    with pytest.raises(NotImplementedError):
        m(i, o)
    with pytest.raises(NotImplementedError):
        m(i, o, per_sample_weights=torch.ones(idx.size))
    # an empty batch is served: zeros, nothing counted
    before = m.cache_freq.clone()
    out = m(torch.zeros(0, dtype=torch.int64), torch.zeros(NT * B + 1, dtype=torch.int64))
    assert out.shape == (NT, B, D_) and not bool(out.any()) and torch.equal(before, m.cache_freq)
    # one table: write_back is still there
    one = bags(ops, num_tables=1, use_cache=True, cache_size=16, hashtbl_size=64)
    one(torch.from_numpy(idx[:4]), torch.tensor([0, 1, 2, 3, 4]))
    one.cache_populate(write_back=0.1)
    assert not one.warmup
