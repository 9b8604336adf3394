"""CPU tests (no GPU) of the cache refresh, `cache_populate(keep_trained=, freq_shift=)`: the C ABI of
ttx_cache_carry (declared, exported by both libraries, argument checks with pointers that are never dereferenced), the
compiler's resource report of csrc/ttx_cache_carry.hip, the numpy restatement tests/carry_ref.py on hand-made arrays, and -- on
top of the oracle engine -- what the modules accept, refuse and leave unchanged."""
import copy
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import carry_ref as CR
import oracle_engine
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


# ----------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_point_is_declared_and_exported_and_checks_its_arguments():
    text = open(os.path.join(ROOT, "include", "ttx.h")).read()
    assert "cache refresh: trained rows across a re-populate (not in the reference)" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ttx_cache_carry\s*\(\s*int64_t hashtbl_size,\s*const int64_t\*\s*hashtbl,\s*const int32_t\*\s*old_state,"
                     r"\s*const int32_t\*\s*cache_state,\s*int64_t cache_size,\s*int32_t D,\s*const float\*\s*old_weight,"
                     r"\s*float\*\s*cache_weight,\s*int32_t state_width,\s*const float\*\s*old_opt_state,\s*float\*\s*opt_state,"
                     r"\s*ttx_stream_t stream\)", hdr), "ttx_cache_carry is not declared"
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    D = 12
    # (never dereferenced: every call below returns before a launch)
    ok = dict(H=64, ht=vp(4096), os=vp(8192), st=vp(12288), cs=16, D=D, ow=vp(1 << 20), cw=vp(2 << 20), sw=0, oo=None, oq=None)
    state1 = dict(sw=1, oo=vp(3 << 20), oq=vp(4 << 20))
    stateD = dict(sw=D, oo=vp(3 << 20), oq=vp(4 << 20))
    bad = [dict(H=0), dict(H=-1), dict(H=1 << 31),                                       # hashtbl_size in (0, 2^31)
           dict(cs=-1), dict(cs=65), dict(D=0), dict(D=-4),                              # cache_size in [0, H]; D > 0
           dict(sw=2), dict(sw=-1), dict(sw=D + 1), dict(state1, sw=D - 1),              # state_width in {0, 1, D}
           dict(ht=None), dict(os=None), dict(st=None), dict(ow=None), dict(cw=None),    # NULL that would be read / written
           dict(sw=1), dict(sw=D), dict(state1, oo=None), dict(state1, oq=None), dict(stateD, oo=None), dict(stateD, oq=None),
           dict(ow=vp(2 << 20)), dict(ow=vp((2 << 20) + 4)), dict(ow=vp((2 << 20) - 16 * D * 4 + 4)),  # the weights overlap
           dict(state1, oo=vp(4 << 20)), dict(state1, oo=vp((4 << 20) + 60)), dict(stateD, oo=vp((4 << 20) + 4 * D)),
           dict(ht=vp(4100)),                                                            # int64 pointer, 8-byte aligned
           dict(os=vp(8194)), dict(st=vp(12290)), dict(ow=vp((1 << 20) + 2)), dict(cw=vp((2 << 20) + 1)), dict(state1, oq=vp((4 << 20) + 2))]
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        carry = lib.ttx_cache_carry
        #                H    ht  os  st  cs   D    ow  cw  sw   oo  oq  stream
        carry.argtypes = [i64, vp, vp, vp, i64, i32, vp, vp, i32, vp, vp, vp]

        def call(a):
            return carry(a["H"], a["ht"], a["os"], a["st"], a["cs"], a["D"], a["ow"], a["cw"], a["sw"], a["oo"], a["oq"], None)

        for change in bad:
            assert call(dict(ok, **change)) == -1, (so, change)
            assert b"cache_carry" in lib.ttx_last_error(), lib.ttx_last_error()
        # nothing to do: 0, and nothing touches a device (no buffers at all) ...
        none = dict(ht=None, os=None, st=None, ow=None, cw=None)
        assert call(dict(ok, cs=0, **none)) == 0
        assert call(dict(ok, cs=0, sw=1, **none)) == 0
        # ... but the argument errors come first
        assert call(dict(ok, cs=0, H=0, **none)) == -1
        assert call(dict(ok, cs=0, sw=5, **none)) == -1


def test_shim_exposes_the_call_and_refuses_cpu_tensors():
    import tt_embeddings as E

    par = inspect.signature(E.cache_carry).parameters
    assert list(par) == ["hashtbl", "old_state", "cache_state", "old_weight", "cache_weight", "old_opt_state", "opt_state"]
    assert par["old_opt_state"].default is None and par["opt_state"].default is None
    assert list(inspect.signature(E.cache_populate).parameters)[-1] == "reference_exact"  # (nothing existing changed its signature)
    ht, st, w = torch.full((8,), -1, dtype=torch.int64), torch.full((8,), -1, dtype=torch.int32), torch.zeros(4, 4)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.cache_carry(ht, st, st.clone(), w, w.clone())
    assert not hasattr(oracle_engine, "cache_carry"), "the tests' oracle engine stays as it is"


def test_module_signatures():
    import tt_embeddings_ops as ops
    import ttx_mixed

    want = ["self", "write_back", "write_back_steps", "keep_trained", "freq_shift"]
    for cls in (ops.TableBatchedTTEmbeddingBag, ops.TTEmbeddingBag, ops.TTEmbedding, ttx_mixed.VarTableTTEmbeddingBag):
        par = inspect.signature(cls.cache_populate).parameters
        assert list(par) == want, cls
        assert (par["write_back"].default, par["write_back_steps"].default, par["keep_trained"].default, par["freq_shift"].default) \
            == (0.0, 1, False, 0), cls
    par = inspect.signature(ttx_mixed.MixedTTEmbeddingBag.cache_populate).parameters
    assert list(par) == ["self", "keep_trained", "freq_shift"] and par["keep_trained"].default is False and par["freq_shift"].default == 0


def test_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed)"""
    from test_kernel_resources import resources

    res = {k: v for k, v in resources("ttx_cache_carry.hip").items() if "kernel" in k}
    assert len(res) == 2 and all("cache_carry_kernel" in k for k in res), sorted(res)  # (16-byte units, floats)
    for k, r in res.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8, (k, r)  # (a copy hides latency with waves in flight)
        assert r.get("LDS Size", r.get("LDSSize", 0)) == 256 * 8 + 16, (k, r)  # (the tile's participants, the waves' counts)


# ----------------------------------------------------------------------------------------------- the reference's properties
def seated(keys, H):
    """a table that holds `keys` where the library's insert puts them -> (hashtbl, {key: slot})"""
    tbl, val = np.full(H, -1, np.int64), np.zeros(H, np.int64)
    slot = {int(k): O.hashtbl_insert(int(k), 1, tbl, val) for k in keys}
    assert all(s >= 0 for s in slot.values())
    return tbl, slot


def rows(cs, D, seed):
    return np.random.RandomState(seed).rand(cs, D).astype(np.float32)


def test_reference_swap_cycle():
    """two keys trade rows, a third walks on: every row comes from the OLD array (in place, the second copy would read the first's
    result)"""
    tbl, slot = seated([5, 9, 11], 64)
    a, b, c = slot[5], slot[9], slot[11]
    old, new = np.full(64, -1, np.int32), np.full(64, -1, np.int32)
    old[[a, b, c]], new[[a, b, c]] = [0, 1, 2], [1, 0, 3]
    ow, cw, oo, oq = rows(5, 6, 1), rows(5, 6, 2), rows(5, 1, 3)[:, 0], rows(5, 1, 4)[:, 0]
    w, st = CR.carry_ref(tbl, old, new, ow, cw, oo, oq)
    assert np.array_equal(w[[1, 0, 3]], ow[[0, 1, 2]]) and np.array_equal(st[[1, 0, 3]], oo[[0, 1, 2]])
    assert np.array_equal(w[[2, 4]], cw[[2, 4]]) and np.array_equal(st[[2, 4]], oq[[2, 4]]), "rows without an owner"
    assert CR.participants(tbl, old, new, 5) == sorted([(a, 1, 0), (b, 0, 1), (c, 3, 2)])
    # element-wise state, and none at all
    oo2, oq2 = rows(5, 6, 5), rows(5, 6, 6)
    w2, st2 = CR.carry_ref(tbl, old, new, ow, cw, oo2, oq2)
    assert np.array_equal(w2, w) and np.array_equal(st2[[1, 0, 3]], oo2[[0, 1, 2]]) and np.array_equal(st2[[2, 4]], oq2[[2, 4]])
    w3, st3 = CR.carry_ref(tbl, old, new, ow, cw)
    assert np.array_equal(w3, w) and st3 is None


def test_reference_ignores_the_second_copy_of_a_key():
    """a key sits in two slots of its probe window; the later copy's stale state names a row another key owns now"""
    H = 64
    tbl, slot = seated([5, 9], H)
    s = slot[5]
    assert s == O.hash64(5, H) and tbl[(s + 1) % H] == -1, "precondition: key 5 at its home slot, the next slot free"
    dup = (s + 1) % H
    tbl[dup] = 5
    assert O.hashtbl_find(5, tbl) == s
    old, new = np.full(H, -1, np.int32), np.full(H, -1, np.int32)
    old[s], new[s] = 2, 0          # key 5: row 2 -> row 0
    old[slot[9]], new[slot[9]] = -1, 1  # key 9: admitted to row 1
    old[dup], new[dup] = 3, 1      # the stale copy claims row 1 with old row 3
    ow, cw, oo, oq = rows(4, 4, 1), rows(4, 4, 2), rows(4, 1, 3)[:, 0], rows(4, 1, 4)[:, 0]
    w, st = CR.carry_ref(tbl, old, new, ow, cw, oo, oq)
    assert np.array_equal(w[0], ow[2]) and st[0] == oo[2]
    assert np.array_equal(w[1], cw[1]) and st[1] == 0, "the admitted key keeps its decompressed row and starts from zero state"
    assert np.array_equal(w[2:], cw[2:]) and np.array_equal(st[2:], oq[2:])
    assert [p[0] for p in CR.participants(tbl, old, new, 4)] == sorted([s, slot[9]])


def test_reference_out_of_range_states_and_empty_slots():
    H, cs = 64, 4
    tbl, slot = seated([3, 4, 6, 7, 8], H)
    old, new = np.full(H, -1, np.int32), np.full(H, -1, np.int32)
    new[slot[3]], old[slot[3]] = 0, cs        # old state >= cache_size: admitted
    new[slot[4]], old[slot[4]] = 1, -5        # old state < 0: admitted
    new[slot[6]], old[slot[6]] = cs, 1        # new state >= cache_size: takes no part
    new[slot[7]], old[slot[7]] = -3, 2        # new state < 0: takes no part
    new[slot[8]], old[slot[8]] = 3, 0         # kept
    empty = next(i for i in range(H) if tbl[i] == -1)
    new[empty], old[empty] = 2, 1             # an empty slot with states in range: takes no part
    ow, cw, oo, oq = rows(cs, 5, 1), rows(cs, 5, 2), rows(cs, 5, 3), rows(cs, 5, 4)
    w, st = CR.carry_ref(tbl, old, new, ow, cw, oo, oq)
    assert np.array_equal(w[[0, 1, 2]], cw[[0, 1, 2]]) and np.array_equal(w[3], ow[0])
    assert not st[[0, 1]].any() and np.array_equal(st[2], oq[2]) and np.array_equal(st[3], oo[0])
    for arr, keep in ((ow, rows(cs, 5, 1)), (cw, rows(cs, 5, 2)), (oo, rows(cs, 5, 3)), (oq, rows(cs, 5, 4))):
        assert np.array_equal(arr, keep), "the reference returns new arrays"


# -------------------------------------------------------------------------------------------------------------- the modules
P, Q, R = [4, 5, 5], [2, 3, 2], [4, 5]
E_, D_, B, LP = 100, 12, 16, 4


def module(ops, **kw):
    torch.manual_seed(2)
    kw.setdefault("optimizer", ops.OptimType.SGD)
    return ops.TTEmbeddingBag(E_, D_, R, P, Q, sparse=True, learning_rate=0.05, use_cache=True, cache_size=20, hashtbl_size=256,
                              weight_dist="uniform", device="cpu", **kw)


def counted(ops, **kw):
    """a module that has counted three batches and populated once, then counted two more"""
    m = module(ops, **kw)
    rs = np.random.RandomState(3)
    off = torch.arange(0, B * LP + 1, LP)
    for step in range(5):
        if step == 3:
            m.cache_populate()
        m.update_cache(torch.from_numpy((rs.zipf(1.3, size=B * LP) % E_).astype(np.int64)), off)
    return m


def arrays(m):
    out = [m.hashtbl, m.cache_freq, m.cache_state, m.cache_weight.detach()] + [c.detach() for c in m.tt_cores]
    return [a.clone() for a in out + ([] if m.cache_optimizer_state is None else [m.cache_optimizer_state])]


def same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def test_the_two_refusals_change_nothing(ops):
    m = counted(ops, reference_exact_populate=True)
    before = arrays(m)
    with pytest.raises(ValueError, match="reference_exact_populate"):
        m.cache_populate(keep_trained=True)
    assert same(arrays(m), before)
    m.cache_populate(freq_shift=1)  # (the ageing alone goes with the reference's populate)
    m = counted(ops)
    before = arrays(m)
    with pytest.raises(NotImplementedError, match="keep_trained"):  # CPU tensors, and an engine without cache_carry
        m.cache_populate(keep_trained=True)
    with pytest.raises(NotImplementedError, match="keep_trained"):
        m.cache_populate(keep_trained=True, freq_shift=1)
    assert same(arrays(m), before) and not m.warmup
    w = module(ops)  # still warming up: refused all the same (the call would be refused on the next populate too)
    with pytest.raises(NotImplementedError):
        w.cache_populate(keep_trained=True)
    assert w.warmup
    u = ops.TTEmbeddingBag(E_, D_, R, P, Q, sparse=True, use_cache=False, weight_dist="uniform", device="cpu")
    u.cache_populate(keep_trained=True, freq_shift=3)  # no cache: nothing to do, as before


def test_unpooled_and_several_tables_take_the_keywords(ops):
    import ttx_mixed

    e = ops.TTEmbedding(E_, D_, R, P, Q, use_cache=True, cache_size=20, hashtbl_size=256, weight_dist="uniform", device="cpu")
    with pytest.raises(NotImplementedError, match="keep_trained"):
        e.cache_populate(keep_trained=True)
    with pytest.raises(ValueError, match="freq_shift"):
        e.cache_populate(freq_shift=63)
    tb = ops.TableBatchedTTEmbeddingBag(3, E_, D_, R, P, Q, sparse=False, use_cache=True, cache_size=20, hashtbl_size=256,
                                        weight_dist="uniform", device="cpu")
    var = ttx_mixed.VarTableTTEmbeddingBag([E_, 60], D_, R, [P, [3, 4, 5]], Q, sparse=False, use_cache=True, cache_size=20,
                                           hashtbl_size=256, weight_dist="uniform", device="cpu")
    mixed = ttx_mixed.MixedTTEmbeddingBag([E_, 60], D_, R, [P, [3, 4, 5]], Q, sparse=False, fused=True, use_cache=True,
                                          cache_size=20, hashtbl_size=256, weight_dist="uniform", device="cpu")
    for m in (tb, var, mixed):
        with pytest.raises(ValueError, match="freq_shift"):
            m.cache_populate(freq_shift=-1)
        with pytest.raises(NotImplementedError, match="keep_trained"):
            m.cache_populate(keep_trained=True)
        with pytest.raises(NotImplementedError):  # (unchanged: these caches are populated on the GPU only)
            m.cache_populate(freq_shift=1)
    for g in (tb, var, mixed.groups[0]):
        assert g.warmup and int(g.cache_freq.sum()) == 0


def test_freq_shift_range(ops):
    m = counted(ops)
    before = arrays(m)
    for bad in (-1, 63, 64, 1.5, "1", None, True):
        with pytest.raises(ValueError, match="freq_shift"):
            m.cache_populate(freq_shift=bad)
    assert same(arrays(m), before)
    m.cache_populate(freq_shift=62)  # the largest shift: every count becomes 0
    assert int(m.cache_freq.sum()) == 0
    counted(ops).cache_populate(freq_shift=np.int64(1))


def test_freq_shift_equals_a_manual_shift(ops):
    m = counted(ops)
    twin = copy.deepcopy(m)
    assert int((m.cache_freq & 3).ne(0).sum()) > 0, "precondition: the shift drops set bits"
    m.cache_populate(freq_shift=2)
    twin.cache_freq >>= 2
    twin.cache_populate()
    assert same(arrays(m), arrays(twin))
    plain = counted(ops)
    plain.cache_populate()
    assert not torch.equal(plain.cache_freq, m.cache_freq)


@pytest.mark.parametrize("optimizer", ["SGD", "EXACT_ROWWISE_ADAGRAD", "EXACT_ADAGRAD"])
def test_defaults_equal_todays_populate(ops, optimizer):
    """cache_populate() and cache_populate(keep_trained=False, freq_shift=0) leave every array as the engine's populate on the
    module's arrays does -- the state included, which no populate touches"""
    m = counted(ops, optimizer=getattr(ops.OptimType, optimizer))
    if m.cache_optimizer_state is not None:
        m.cache_optimizer_state.copy_(torch.rand_like(m.cache_optimizer_state))
    a, b = copy.deepcopy(m), copy.deepcopy(m)
    m.cache_populate()
    a.cache_populate(keep_trained=False, freq_shift=0)
    oracle_engine.cache_populate(b.num_embeddings, b.tt_p_shapes, b.tt_q_shapes, b.tt_ranks, list(b.tt_cores), b.L, b.hashtbl,
                                 b.cache_freq, b.cache_state, b.cache_weight)
    assert same(arrays(m), arrays(b)) and same(arrays(a), arrays(b))
