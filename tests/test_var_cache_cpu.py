"""CPU tests (no GPU) of the row cache over tables of DIFFERENT row factors, `VarTableTTEmbeddingBag(use_cache=True)` and
`MixedTTEmbeddingBag(fused=True, use_cache=True)`: the C ABI of ttx_table_keys_v / ttx_table_keys_split_v /
ttx_cache_populate_v (declared, exported by both libraries, argument checks with pointers that are never dereferenced), the shim's
calls, the compiler's resource report of csrc/ttx_cache_vtables.hip, and -- on top of the oracle engine, with the per-table
lookup stated in torch by tests/test_mixed_modes_cpu.py -- what the modules accept, count and refuse."""
import collections
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from test_mixed_modes_cpu import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, R, D_ = [2, 2, 3], [4, 3], 12
ES = [24, 210, 60]                          # three cardinalities; table 1 is looked up at local indices >= 24
PS = [[2, 3, 4], [5, 6, 7], [3, 4, 5]]
BASES = [0, 24, 24 + 210, 24 + 210 + 60]    # prod(p) of the tables, summed up
NT, B = 3, 4


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", Engine())
    return m


def var(ops, Es=ES, ps=PS, **kw):
    import ttx_mixed

    kw.setdefault("sparse", False)
    torch.manual_seed(3)
    return ttx_mixed.VarTableTTEmbeddingBag(Es, D_, R, ps, Q, weight_dist="uniform", device="cpu", **kw)


# ----------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_and_exported_and_check_their_arguments():
    text = open(os.path.join(ROOT, "include", "ttx.h")).read()
    assert "row cache over tables of different row factors (not in the reference)" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ttx_table_keys_v\s*\(\s*int64_t nnz,\s*const int64_t\*\s*indices,\s*int32_t num_tables,\s*int64_t B,"
                     r"\s*const int64_t\*\s*offsets,\s*const int64_t\*\s*key_base,\s*int64_t\*\s*keys,\s*int64_t H,"
                     r"\s*int64_t\*\s*upd_hashtbl,\s*int64_t\*\s*upd_cache_freq,\s*ttx_stream_t stream\)", hdr), "ttx_table_keys_v"
    assert re.search(r"\bint\s+ttx_table_keys_split_v\s*\(\s*int64_t n,\s*const int32_t\*\s*n_dev,\s*int32_t num_tables,\s*int64_t B,"
                     r"\s*const int64_t\*\s*key_base,\s*const int64_t\*\s*keys,\s*const int64_t\*\s*bagrow,\s*int64_t\*\s*out_indices,"
                     r"\s*int64_t\*\s*out_tableidx,\s*int64_t\*\s*out_rowidx,\s*ttx_stream_t stream\)", hdr), "ttx_table_keys_split_v"
    assert re.search(r"\bint\s+ttx_cache_populate_v\s*\(\s*const ttx_geom\*\s*g,", hdr), "ttx_cache_populate_v is not declared"
    assert re.search(r"\bsize_t\s+ttx_cache_populate_v_workspace_bytes\s*\(", hdr)
    i64, i32, vp, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_size_t
    fake, odd4, odd2 = vp(4096), vp(4100), vp(4098)  # (never dereferenced: every call below returns before a launch)
    import tt_embeddings as E

    def arr(vals):
        return (i64 * len(vals))(*vals)

    ranks = [1] + R + [1]
    mixed = E._geom(NT, PS, Q, ranks)
    uniform = E._geom(NT, PS[1], Q, ranks)
    one = E._geom(1, [PS[1]], Q, ranks)  # (one table with per-table factors: make_dims needs no device for it)
    two_cores = E._geom(2, [[4, 5], [6, 7]], [3, 4], [1, 6, 1])
    four_cores = E._geom(2, [[4, 5, 3, 4], [3, 4, 5, 2]], [2, 2, 2, 2], [1, 3, 3, 3, 1])
    huge = E._geom(2, [[1 << 21, 1 << 20, 1 << 20]] * 2, Q, ranks)  # 2 x 2^61 keys
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        keys, split, pop = lib.ttx_table_keys_v, lib.ttx_table_keys_split_v, lib.ttx_cache_populate_v
        #               nnz  idx nt   B    off base keys H   hashtbl freq stream
        keys.argtypes = [i64, vp, i32, i64, vp, vp, vp, i64, vp, vp, vp]
        #                n    dev nt   B    base keys bagrow idx tab row stream
        split.argtypes = [i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
        #              g   cores H   ht  freq state cs  D    cw  flags ws  bytes stream
        pop.argtypes = [vp, vp, i64, vp, vp, vp, i64, i32, vp, i32, vp, sz, vp]
        base, shifted = arr(BASES), arr([0] + BASES + [0])
        # nothing to do: 0, and nothing touches a device (no buffers at all)
        assert keys(0, None, NT, B, None, base, None, 0, None, None, None) == 0
        assert split(0, None, NT, B, base, None, None, None, None, None, None) == 0
        bad_bases = [dict(base=None), dict(base=arr([1, 24, 234, 294])),                  # NULL; does not start at 0
                     dict(base=arr([0, 24, 24, 294])), dict(base=arr([0, 234, 24, 294])),   # not strictly increasing
                     dict(base=arr([0, 24, 234, 1 << 62])),                                # ends at 2^62
                     dict(base=vp(ctypes.addressof(shifted) + 4))]                         # not 8-byte aligned
        ok = dict(nnz=8, idx=fake, nt=NT, B=B, off=fake, base=base, keys=fake, H=64, ht=fake, freq=fake)
        bad_keys = [dict(nnz=-1), dict(nnz=1 << 31),                                     # negative size, nnz >= 2^31
                    dict(B=0), dict(B=-3), dict(nt=0), dict(nt=-1), dict(nt=65),
                    dict(nt=64, B=1 << 26, base=arr(list(range(65)))),                    # 2^32 bags
                    dict(idx=None), dict(off=None), dict(keys=None),                      # NULL that would be read / written
                    dict(ht=None), dict(freq=None), dict(H=0), dict(H=1 << 31),           # counting: both tables, H in (0, 2^31)
                    dict(idx=odd4), dict(off=odd4), dict(keys=odd4), dict(ht=odd4), dict(freq=odd4)] + bad_bases
        for change in bad_keys:
            a = dict(ok, **change)
            rc = keys(a["nnz"], a["idx"], a["nt"], a["B"], a["off"], a["base"], a["keys"], a["H"], a["ht"], a["freq"], None)
            assert rc == -1, ("ttx_table_keys_v", so, change)
            assert b"table_keys_v" in lib.ttx_last_error(), lib.ttx_last_error()
        # the argument errors come first: a bad size is refused for an empty batch too
        assert keys(0, None, NT, 0, None, base, None, 0, None, None, None) == -1
        assert keys(0, None, NT, B, None, arr([0, 5, 5, 9]), None, 0, None, None, None) == -1
        # 64 tables, one of stride 1, a key space just below 2^62: accepted (nothing to launch)
        wide = arr([0, 1] + [2 + k * (1 << 50) for k in range(62)] + [(1 << 62) - 1])
        assert keys(0, None, 64, B, None, wide, None, 0, None, None, None) == 0, lib.ttx_last_error()
        oks = dict(n=8, dev=None, nt=NT, B=B, base=base, keys=fake, bagrow=fake, idx=fake, tab=fake, row=fake)
        bad_split = [dict(n=-1), dict(n=1 << 31), dict(B=0), dict(nt=0), dict(nt=65),
                     dict(nt=64, B=1 << 26, base=arr(list(range(65)))),
                     dict(keys=None), dict(idx=None), dict(tab=None), dict(row=None),   # (row: written when bagrow is given)
                     dict(bagrow=None, idx=None),
                     dict(dev=odd2), dict(keys=odd4), dict(bagrow=odd4), dict(idx=odd4), dict(tab=odd4), dict(row=odd4)] + bad_bases
        for change in bad_split:
            a = dict(oks, **change)
            rc = split(a["n"], a["dev"], a["nt"], a["B"], a["base"], a["keys"], a["bagrow"], a["idx"], a["tab"], a["row"], None)
            assert rc == -1, ("ttx_table_keys_split_v", so, change)
            assert b"table_keys_split_v" in lib.ttx_last_error(), lib.ttx_last_error()
        mp, up, op = ctypes.addressof(mixed), ctypes.addressof(uniform), ctypes.addressof(one)
        okp = dict(g=mp, cores=fake, H=64, ht=fake, freq=fake, state=fake, cs=16, D=D_, cw=fake, flags=0, ws=fake, bytes=1 << 30)
        bad_pop = [dict(g=None), dict(g=up),                                            # no geometry; no per-table row factors
                   dict(g=ctypes.addressof(huge)),                                      # a key space of 2^62
                   dict(H=0), dict(H=-1), dict(H=1 << 31), dict(cs=-1), dict(cs=65), dict(D=0), dict(flags=2),
                   dict(cores=None), dict(ht=None), dict(freq=None), dict(state=None), dict(cw=None),
                   dict(ht=odd4), dict(freq=odd4), dict(state=odd2), dict(cw=odd2), dict(ws=odd4)]
        for change in bad_pop:
            a = dict(okp, **change)
            rc = pop(a["g"], a["cores"], a["H"], a["ht"], a["freq"], a["state"], a["cs"], a["D"], a["cw"], a["flags"], a["ws"],
                     a["bytes"], None)
            assert rc == -1, ("ttx_cache_populate_v", so, change)
            assert b"cache_populate_v" in lib.ttx_last_error(), lib.ttx_last_error()
        for g in (two_cores, four_cores):  # three cores only: TTX_EUNSUPPORTED
            rc = pop(ctypes.addressof(g), fake, 64, fake, fake, fake, 16, 12, fake, 0, fake, 1 << 30, None)
            assert rc == -3 and b"three TT cores" in lib.ttx_last_error(), lib.ttx_last_error()
        rc = pop(op, fake, 64, fake, fake, fake, 16, D_, fake, 0, None, 0, None)  # no workspace: refused before a launch
        assert rc == -2, lib.ttx_last_error()
        lib.ttx_cache_populate_v_workspace_bytes.restype = sz
        lib.ttx_cache_populate_v_workspace_bytes.argtypes = [vp, i64, i64, i32]
        assert lib.ttx_cache_populate_v_workspace_bytes(op, 64, 16, D_) > 4 * 64 * 8 + 2 * 16 * 8
        assert lib.ttx_cache_populate_v_workspace_bytes(up, 64, 16, D_) == 0
        assert lib.ttx_cache_populate_v_workspace_bytes(ctypes.addressof(two_cores), 64, 16, 12) == 0


def test_engine_takes_key_bases_in_the_place_of_the_stride():
    import tt_embeddings as E

    # (nothing existing changed its signature: an int keeps today's call)
    assert list(inspect.signature(E.table_keys).parameters) == ["indices", "offsets", "num_tables", "key_stride", "hashtbl", "cache_freq"]
    assert list(inspect.signature(E.table_keys_split).parameters) == ["keys", "bagrow", "num_tables", "B", "key_stride", "n_dev"]
    assert list(inspect.signature(E.cache_populate_var_tables).parameters) == [
        "tt_p_shapes", "tt_q_shapes", "tt_ranks", "tt_cores", "hashtbl", "cache_freq", "cache_state", "cache_weight", "reference_exact"]
    assert inspect.signature(E.cache_populate_var_tables).parameters["reference_exact"].default is False
    assert E.key_bases_of(PS) == BASES
    assert E._key_bases(7, 3) is None and E._key_bases(np.int64(7), 3) is None
    assert list(E._key_bases(BASES, 3)) == BASES
    with pytest.raises(RuntimeError, match="key bases"):
        E._key_bases(BASES[:-1], 3)
    i64 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.table_keys(i64, torch.arange(4), 3, BASES)
    with pytest.raises(RuntimeError):
        E.table_keys_split(i64, i64, 3, 1, BASES)


def test_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed)"""
    from test_kernel_resources import resources

    res = {k: v for k, v in resources("ttx_cache_vtables.hip").items() if "kernel" in k}
    assert len(res) == 2 and all(any(w in k for k in res) for w in ("table_keys_v_kernel", "table_keys_split_v_kernel")), sorted(res)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs Spill"] == 0 and r["SGPRs Spill"] == 0, (k, r)
        lds = r.get("LDS Size", r.get("LDSSize", 0))
        assert lds <= 2 * 65 * 8 + 16, (k, r)  # (the staged key bases, and the table boundaries: 65 int64 each)


# -------------------------------------------------------------------------------------------------------------- the modules
def test_constructor_builds_the_one_table_modules_state(ops):
    kw = dict(use_cache=True, cache_size=16, hashtbl_size=64, optimizer=ops.OptimType.EXACT_ROWWISE_ADAGRAD, sparse=True)
    m = var(ops, **kw)
    torch.manual_seed(3)
    one = ops.TableBatchedTTEmbeddingBag(1, ES[1], D_, R, PS[1], Q, weight_dist="uniform", device="cpu", **kw)
    assert list(m.state_dict()) == list(one.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in one.named_parameters()]
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in one.named_buffers()]
    for k, v in m.state_dict().items():  # one cache for all tables: only the cores (and their state) hold the tables' slices
        w = one.state_dict()[k]
        assert tuple(v.shape) == tuple(w.shape) or (v.dim() == 3 and v.shape[0] == 1 and v.shape[2] == w.shape[2]), k
    assert m.warmup and m.use_cache and m.cache_weight.shape == (16, D_) and m.hashtbl.numel() == 64
    assert m.cache_optimizer_state.shape == (16,)
    assert m._key_space() == BASES and m._tables_cache()
    assert var(ops, use_cache=True, optimizer=ops.OptimType.EXACT_ADAGRAD, sparse=True, cache_size=8).cache_optimizer_state.shape == (8, D_)
    assert var(ops, use_cache=True, cache_size=8).cache_optimizer_state is None
    plain = var(ops)
    assert not plain.use_cache and plain.cache_weight is None and plain.hashtbl.numel() == 0 and not plain._tables_cache()


def test_defaults_and_errors(ops):
    import ttx_mixed

    m = var(ops, use_cache=True)
    assert m.cache_weight.size(0) == int(0.1 * sum(ES)) and m.hashtbl.numel() == sum(ES) == m.cache_freq.numel() == m.cache_state.numel()
    assert m.deterministic_cache_update is None and m.reference_exact_populate is False
    m = var(ops, use_cache=True, deterministic_cache_update=True, reference_exact_populate=True)
    assert m.deterministic_cache_update is True and m.reference_exact_populate is True
    with pytest.raises(ValueError, match="hashtbl_size"):
        var(ops, use_cache=True, cache_size=8, hashtbl_size=1 << 31)
    with pytest.raises(ValueError, match="hashtbl_size"):  # the default, the sum of the cardinalities, can be too large too
        var(ops, Es=[1 << 30, 1 << 30], ps=[[1 << 10] * 3] * 2, use_cache=True, cache_size=8)
    with pytest.raises(ValueError, match="key space"):
        var(ops, Es=[100, 100], ps=[[1 << 21, 1 << 20, 1 << 20]] * 2, use_cache=True, cache_size=8, hashtbl_size=64)
    with pytest.raises(NotImplementedError, match="max"):
        var(ops, use_cache=True, mode="max")
    with pytest.raises(NotImplementedError, match="table_q"):
        ttx_mixed.VarTableTTEmbeddingBag(ES, D_, R, PS, [2, 3, 3], weight_dist="uniform", device="cpu", sparse=False,
                                         table_q=[[2, 2, 3], [2, 3, 2], [2, 2, 3]], use_cache=True)
    for ps, q, r in (([[5, 8], [6, 7]], [3, 4], [6]), ([[4, 5, 3, 4], [3, 4, 5, 2]], [2, 2, 2, 2], [3, 3, 3])):
        Es = [int(np.prod(p)) for p in ps]
        kw = dict(weight_dist="uniform", device="cpu", sparse=False)
        ttx_mixed.VarTableTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, **kw)
        with pytest.raises(NotImplementedError, match="three TT cores"):
            ttx_mixed.VarTableTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, use_cache=True, **kw)


def batch(seed, empty_table=None):
    """NT * B bags of 0 .. 4 lookups, table-major; bag 1 of table 0 is empty, `empty_table` has no lookups at all.  Table 0 draws
    from 0 .. 9 (hot), table 1 from 0 .. 9 as well and from 24 .. 209 (beyond table 0's cardinality), table 2 from 0 .. 59"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(0, 5, size=NT * B)
    lens[1] = 0
    lens[B] = 4
    if empty_table is not None:
        lens[empty_table * B:(empty_table + 1) * B] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    table = np.repeat(np.arange(NT * B) // B, lens)
    idx = np.empty(table.size, np.int64)
    for n, k in enumerate(table):
        idx[n] = rs.randint(0, 10) if k == 0 or (k == 1 and n % 2) else rs.randint(24, 210) if k == 1 else rs.randint(0, 60)
    return idx, off, idx + np.asarray(BASES)[table], table


def freq_map(m):
    ht, fr = m.hashtbl.numpy(), m.cache_freq.numpy()
    return {int(k): int(v) for k, v in zip(ht[ht >= 0], fr[ht >= 0])}


def test_cpu_warm_up_counts_keys(ops):
    """two batches -- one with a table that has no lookups -- on a table of 4096 slots for well under 100 distinct keys (the
    oracle's insert drops a key after three probes: asserted not to happen)"""
    m = var(ops, use_cache=True, cache_size=16, hashtbl_size=4096)
    twin = var(ops)
    with torch.no_grad():
        for dst, src in zip(twin.tt_cores, m.tt_cores):
            dst.copy_(src)
    want = collections.Counter()
    n = 0
    seen1 = []
    for seed, empty in ((5, None), (6, 2)):
        idx, off, keys, table = batch(seed, empty)
        out = m(torch.from_numpy(idx), torch.from_numpy(off))
        assert out.shape == (NT, B, D_)
        assert torch.equal(out, twin(torch.from_numpy(idx), torch.from_numpy(off))), "counting changes nothing else"
        want.update(keys.tolist())
        n += idx.size
        seen1 += idx[table == 1].tolist()
    assert any(v < 10 for v in seen1) and any(v >= 24 for v in seen1), "table 1: table 0's hot indices, and indices beyond table 0"
    got = freq_map(m)
    assert sum(got.values()) == n, "a key ran out of probes"
    assert got == dict(want)
    tables = {int(np.searchsorted(BASES, k, side="right")) - 1 for k in got}
    assert tables == {0, 1, 2}
    local = collections.defaultdict(set)  # the same local index under two tables is two keys
    for k in got:
        tb = int(np.searchsorted(BASES, k, side="right")) - 1
        local[k - BASES[tb]].add(tb)
    assert any({0, 1} <= v for v in local.values())
    assert m.warmup
    # update_cache(indices, offsets) counts keys too, and needs the offsets
    idx, off, keys, _ = batch(7)
    m.update_cache(torch.from_numpy(idx), torch.from_numpy(off))
    want.update(keys.tolist())
    assert freq_map(m) == dict(want)
    with pytest.raises(ValueError, match="offsets"):
        m.update_cache(torch.from_numpy(idx))
    m.reset_cache()
    assert freq_map(m) == {} and m.warmup and int(m.cache_state.max()) == -1


def test_what_the_cache_refuses_on_cpu_tensors_and_while_live(ops):
    m = var(ops, use_cache=True, cache_size=16, hashtbl_size=64)
    idx, off, _, _ = batch(9)
    i, o = torch.from_numpy(idx), torch.from_numpy(off)
    assert m.prefetch(i, o) is False and m.prefetch_many([(i, o), (i, o)]) is False
    with pytest.raises(NotImplementedError, match="write_back"):
        m.cache_populate(write_back=0.1)
    with pytest.raises(NotImplementedError):  # nothing goes live on the CPU
        m.cache_populate()
    assert m.warmup
    m.warmup = False  # (as if it had)
    assert m.prefetch(i, o) is False and m.prefetch_many([(i, o), (i, o)]) is False
    with pytest.raises(NotImplementedError):
        m(i, o)
    with pytest.raises(NotImplementedError):
        m(i, o, per_sample_weights=torch.ones(idx.size))
    # an empty batch is served: zeros, nothing counted
    before = m.cache_freq.clone()
    out = m(torch.zeros(0, dtype=torch.int64), torch.zeros(NT * B + 1, dtype=torch.int64))
    assert out.shape == (NT, B, D_) and not bool(out.any()) and torch.equal(before, m.cache_freq)
    # a module without a cache: the calls are no-ops
    plain = var(ops)
    plain.cache_populate(), plain.reset_cache(), plain.update_cache(i, o)
    assert plain.warmup


# --------------------------------------------------------------------------------------------------------- MixedTTEmbeddingBag
MES = [24, 210, 60, 500, 90]
MPS = [[2, 3, 4], [5, 6, 7], [3, 4, 5], [8, 8, 8], [4, 5, 5]]
MQS = [[2, 2, 3], [2, 2, 3], [2, 2, 3], [3, 2, 2], [3, 2, 2]]  # two factorings: two fused groups with pad_q=False


def mixed(ops, **kw):
    import ttx_mixed

    torch.manual_seed(5)
    kw.setdefault("sparse", False)
    return ttx_mixed.MixedTTEmbeddingBag(MES, D_, R, MPS, MQS, weight_dist="uniform", device="cpu", fused=True, pad_q=False, **kw)


def test_mixed_splits_the_cache_over_its_groups_and_refuses_what_it_cannot_serve(ops):
    import ttx_mixed

    m = mixed(ops, use_cache=True)
    assert m.group_tables == [[0, 1, 2], [3, 4]] and all(g.use_cache for g in m.groups)
    assert [g.cache_weight.size(0) for g in m.groups] == [int(0.1 * 294), int(0.1 * 590)], "0: every group's default"
    assert [g.hashtbl.numel() for g in m.groups] == [294, 590]
    m = mixed(ops, use_cache=True, cache_size=100, hashtbl_size=1000, deterministic_cache_update=True)
    assert [g.cache_weight.size(0) for g in m.groups] == [100 * 294 // 884, 100 * 590 // 884] == [33, 66]
    assert [g.hashtbl.numel() for g in m.groups] == [1000 * 294 // 884, 1000 * 590 // 884]
    assert all(g.deterministic_cache_update is True for g in m.groups)
    m = mixed(ops, use_cache=True, cache_size=2, hashtbl_size=884)  # rounded down to 0: at least one row per group
    assert [g.cache_weight.size(0) for g in m.groups] == [1, 1]
    assert not any(g.use_cache for g in mixed(ops).groups)
    kw = dict(weight_dist="uniform", device="cpu", sparse=False)
    with pytest.raises(NotImplementedError, match="fused"):
        ttx_mixed.MixedTTEmbeddingBag(MES, D_, R, MPS, MQS, use_cache=True, **kw)
    with pytest.raises(NotImplementedError, match="pad_q=False"):
        ttx_mixed.MixedTTEmbeddingBag(MES, D_, R, MPS, MQS, fused=True, pad_q=True, use_cache=True, **kw)
    ttx_mixed.MixedTTEmbeddingBag(MES, D_, R, MPS, MQS, fused=True, pad_q=True, **kw)  # (without a cache: served)


def test_mixed_fans_the_cache_calls_out_to_its_groups(ops):
    m = mixed(ops, use_cache=True, cache_size=40, hashtbl_size=8192, padding_idx=[None, 3, None, None, 7])
    twin = mixed(ops, padding_idx=[None, 3, None, None, 7])
    rs = np.random.RandomState(11)
    idx, off = [], []
    for e in MES:
        lens = rs.randint(0, 4, size=B)
        lens[1] = 0
        off.append(torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)))
        idx.append(torch.from_numpy(rs.randint(0, min(e, 12), size=int(lens.sum())).astype(np.int64)))
    outs, refs = m(idx, off), twin(idx, off)
    assert all(torch.equal(a, b) for a, b in zip(outs, refs))
    want = [collections.Counter(), collections.Counter()]
    for g, tables in enumerate(m.group_tables):
        bases = m.groups[g]._key_space()
        for j, k in enumerate(tables):
            live = idx[k].numpy()
            if m.padding_idx[k] is not None:
                live = live[live != m.padding_idx[k]]
            want[g].update((live + bases[j]).tolist())
    assert [freq_map(g) for g in m.groups] == [dict(w) for w in want], "the forward counts keys, the padding left out"
    m.update_cache(idx, off)
    assert [freq_map(g) for g in m.groups] == [{k: 2 * v for k, v in w.items()} for w in want]
    with pytest.raises(NotImplementedError):  # the groups' populate is the GPU's
        m.cache_populate()
    m.reset_cache()
    assert [freq_map(g) for g in m.groups] == [{}, {}]
    twin.update_cache(idx, off), twin.cache_populate(), twin.reset_cache()  # (no cache: no-ops)
