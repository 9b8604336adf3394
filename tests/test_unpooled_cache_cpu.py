"""CPU tests (no GPU) of the unpooled lookup with a row cache, `TTEmbedding(use_cache=True)`: the C ABI of ttx_rows_place /
ttx_rows_pick (declared, exported by both libraries, argument checks with pointers that are never dereferenced), the shim's new
calls, the compiler's resource report of csrc/ttx_rows_cache.hip, and -- on top of the oracle engine -- the module after warm-up
and populate against torch's own F.embedding on the expanded table, its state_dict / pickling and its keywords."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_engine
from test_padding_idx_cpu import D_, E_, P, PAD, Q, R
from util import assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ttx_rows_place", "ttx_rows_pick")


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


def emb(ops, **kw):
    kw.setdefault("sparse", False)
    torch.manual_seed(3)
    return ops.TTEmbedding(E_, D_, R, P, Q, weight_dist="uniform", device="cpu", **kw)


def bag(ops, **kw):
    kw.setdefault("sparse", False)
    torch.manual_seed(3)
    return ops.TTEmbeddingBag(E_, D_, R, P, Q, weight_dist="uniform", device="cpu", **kw)


CACHE = dict(use_cache=True, cache_size=32, hashtbl_size=256)


def live(ops, **kw):
    """a module whose cache went live on a stream over 24 hot keys (PAD not among them)"""
    m = emb(ops, **CACHE, **kw)
    hot = np.array([k for k in range(40, 70) if k != PAD][:24], dtype=np.int64)
    rs = np.random.RandomState(2)
    with torch.no_grad():
        for _ in range(3):
            m(torch.from_numpy(hot[rs.randint(0, hot.size, size=(4, 9))]))
    assert m.warmup
    m.cache_populate()
    assert not m.warmup and int((m.cache_state >= 0).sum()) > 0
    return m, hot


def indices_of(shape, hot, seed, padded):
    """half hot keys (hits), half keys never counted (misses); padded: about a third of the positions PAD (0-D: PAD itself)"""
    rs = np.random.RandomState(seed)
    cold = rs.randint(100, E_, size=shape).astype(np.int64)
    idx = np.where(rs.rand(*shape) < 0.5, hot[rs.randint(0, hot.size, size=shape)], cold)
    if padded:
        idx = np.where(rs.rand(*shape) < 0.35, PAD, idx) if shape else np.array(PAD, np.int64)
        if idx.ndim >= 1 and idx.size > 2:
            idx.reshape(-1)[0], idx.reshape(-1)[1] = PAD, hot[0]
    return torch.from_numpy(np.asarray(idx, dtype=np.int64))


# ----------------------------------------------------------------------------------------------------------------- the ABI
def test_entry_points_are_declared_and_exported_and_check_their_arguments():
    text = open(os.path.join(ROOT, "include", "ttx.h")).read()
    assert "unpooled rows with a live cache (not in the reference)" in text
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bint\s+ttx_rows_place\s*\(\s*int64_t N,\s*int64_t n,\s*int64_t n_tt,\s*const int32_t\*\s*n_tt_dev,\s*int32_t D,"
                     r"\s*const int64_t\*\s*pos,\s*const int32_t\*\s*loc,\s*const float\*\s*rows_tt,\s*const float\*\s*cache_weight,"
                     r"\s*int64_t cache_size,\s*const int64_t\*\s*rank,\s*float\*\s*out,", hdr), "ttx_rows_place is not declared"
    assert re.search(r"\bint\s+ttx_rows_pick\s*\(\s*int64_t N,\s*int64_t n,\s*int64_t n_tt,\s*const int32_t\*\s*n_tt_dev,\s*int32_t D,"
                     r"\s*const int64_t\*\s*pos,\s*const float\*\s*d_out,\s*float\*\s*d_rows,", hdr), "ttx_rows_pick is not declared"
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    fake, odd, odd8 = vp(4096), vp(4098), vp(4100)  # (never dereferenced: every call below returns before a launch)
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        place, pick = lib.ttx_rows_place, lib.ttx_rows_pick
        #                 N    n    n_tt dev D    pos loc rows cache cs  rank out stream
        place.argtypes = [i64, i64, i64, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp]
        #                N    n    n_tt dev D    pos d_out d_rows stream
        pick.argtypes = [i64, i64, i64, vp, i32, vp, vp, vp, vp]
        # nothing to move: 0, and nothing touches a device (no buffers at all)
        assert place(0, 0, 0, None, 4, None, None, None, None, 0, None, None, None) == 0
        assert pick(0, 0, 0, None, 4, None, None, None, None) == 0
        ok = dict(N=8, n=8, n_tt=4, dev=None, D=4, pos=fake, loc=fake, rows=fake, cache=fake, cs=16, rank=None, out=fake)
        bad_place = [dict(N=-1, n=0, n_tt=0), dict(n=-1), dict(n_tt=-1),         # negative sizes
                     dict(D=0), dict(D=-4),                                        # D <= 0
                     dict(N=1 << 31, n=1 << 31),                                   # N >= 2^31
                     dict(n=9, rank=fake),                                         # n > N
                     dict(n_tt=9),                                                 # n_tt > n
                     dict(n_tt=9, dev=fake),                                       # ... with a device count too
                     dict(cs=0), dict(cs=-1),                                      # hits with a host count and no cache rows
                     dict(pos=None), dict(loc=None), dict(rows=None), dict(cache=None), dict(out=None),  # NULL that would be read
                     dict(n_tt=8, dev=fake, loc=None), dict(n_tt=8, dev=fake, cache=None),  # a device count may leave hits
                     dict(n=4, n_tt=2),                                            # rank == NULL with n != N
                     dict(rows=odd), dict(cache=odd), dict(out=odd), dict(loc=odd), dict(dev=odd),  # not 4-byte aligned
                     dict(pos=odd8), dict(n=4, n_tt=2, rank=odd8)]                 # int64 pointers not 8-byte aligned
        for change in bad_place:
            a = dict(ok, **change)
            rc = place(a["N"], a["n"], a["n_tt"], a["dev"], a["D"], a["pos"], a["loc"], a["rows"], a["cache"], a["cs"], a["rank"],
                       a["out"], None)
            assert rc == -1, ("ttx_rows_place", so, change)
            assert b"rows_place" in lib.ttx_last_error(), lib.ttx_last_error()
        # pointers that are NOT read may be NULL: all misses need no cache, all hits no rows (these would launch, so: not called)
        okp = dict(N=8, n=8, n_tt=4, dev=None, D=4, pos=fake, d_out=fake, d_rows=fake)
        bad_pick = [dict(N=-1, n=0, n_tt=0), dict(n=-1), dict(n_tt=-1), dict(D=0), dict(D=-4), dict(N=1 << 31, n=1 << 31),
                    dict(n=9), dict(n_tt=9), dict(n_tt=9, dev=fake),
                    dict(pos=None), dict(d_out=None), dict(d_rows=None), dict(n_tt=0, dev=fake, pos=None),
                    dict(d_out=odd), dict(d_rows=odd), dict(dev=odd), dict(pos=odd8)]
        for change in bad_pick:
            a = dict(okp, **change)
            rc = pick(a["N"], a["n"], a["n_tt"], a["dev"], a["D"], a["pos"], a["d_out"], a["d_rows"], None)
            assert rc == -1, ("ttx_rows_pick", so, change)
            assert b"rows_pick" in lib.ttx_last_error(), lib.ttx_last_error()
        # no lookups, or nothing but hits with a host count: nothing to pick, 0 without a launch
        assert pick(8, 0, 0, None, 4, None, None, None, None) == 0
        assert pick(8, 8, 0, None, 4, fake, None, None, None) == 0


def test_engine_exposes_the_calls_and_refuses_cpu_tensors():
    import inspect

    import tt_embeddings as E

    for name in ("rows_place", "rows_pick", "preprocess_indices_async"):
        assert callable(getattr(E, name)), name
    assert list(inspect.signature(E.preprocess_indices_async).parameters) == ["colidx", "offsets", "hashtbl", "cache_state",
                                                                              "update_cache_freq"]
    for f in (E.cache_backward_sgd, E.cache_backward_dense, E.cache_backward_rowwise_adagrad_approx):
        par = inspect.signature(f).parameters
        assert list(par)[-1] == "skip_dev" and par["skip_dev"].default is None, f.__name__
    assert list(inspect.signature(E.make_plan).parameters)[-1] == "n_dev"  # (nothing existing changed its signature)
    i64, i32 = torch.zeros(4, dtype=torch.int64), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.rows_place(4, 2, i64, i32, torch.zeros(4, 8), torch.zeros(3, 8))
    with pytest.raises(RuntimeError):
        E.rows_pick(2, i64, torch.zeros(4, 8))
    with pytest.raises(RuntimeError):
        E.preprocess_indices_async(i64, torch.arange(5), torch.full((16,), -1, dtype=torch.int64), torch.full((16,), -1, dtype=torch.int32))


def test_kernels_use_no_scratch_and_no_lds():
    """the compiler's own resource report for gfx950 (no GPU needed)"""
    from test_kernel_resources import resources

    res = {k: v for k, v in resources("ttx_rows_cache.hip").items() if "kernel" in k}
    assert len(res) == 4 and all(any(w in k for k in res) for w in
                                 ("rc_place4_kernel", "rc_place1_kernel", "rc_pick4_kernel", "rc_pick1_kernel")), sorted(res)
    for k, r in res.items():
        assert "rows_expand" not in k and "rows_collect" not in k, k
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64, (k, r)
        assert r.get("LDS Size", r.get("LDSSize", 0)) == 0, (k, r)


# -------------------------------------------------------------------------------------------------------------- the module
@pytest.mark.parametrize("shape", [(), (7,), (3, 5)], ids=str)
@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_live_forward_equals_torch_embedding_on_the_expanded_table(ops, shape, pad):
    m, hot = live(ops, padding_idx=pad)
    idx = indices_of(shape, hot, seed=4, padded=pad is not None)
    w0 = m.full_weight().detach().clone()  # (the cache rows were decompressed from these cores: the same table)
    if pad is not None:
        w0[pad] = 0
        assert (idx == pad).any()
    out = m(idx)
    assert out.shape == shape + (D_,) and out.dtype == torch.float32
    assert_close(out.detach().numpy(), F.embedding(idx, w0).numpy(), f"cache-live forward {shape}")
    if pad is not None:
        assert (out.detach()[idx == pad] == 0).all(), "padding positions are exact zeros"
    if shape:
        keys = set(m.hashtbl[m.cache_state >= 0].tolist())
        hits = sum(int(v) in keys for v in idx.reshape(-1).tolist() if v != pad)
        assert 0 < hits < int((idx != (-1 if pad is None else pad)).sum()), "the batch must mix hits and misses"


def test_warm_up_counts_live_indices_only(ops):
    m = emb(ops, padding_idx=PAD, **CACHE)
    t = bag(ops, padding_idx=PAD, **CACHE)
    idx = torch.tensor([[PAD, 41, 41], [77, PAD, 41]])
    with torch.no_grad():
        m(idx)
        t(idx.reshape(-1), torch.arange(7))
    pairs = lambda x: sorted(zip(x.hashtbl[x.hashtbl >= 0].tolist(), x.cache_freq[x.hashtbl >= 0].tolist()))  # noqa: E731
    assert pairs(m) == pairs(t) == [(41, 3), (77, 1)]


def test_state_dict_is_the_cached_bag_modules_and_loads_both_ways(ops):
    kw = dict(optimizer=ops.OptimType.EXACT_ADAGRAD, sparse=True)
    e, b = emb(ops, padding_idx=PAD, **CACHE, **kw), bag(ops, **CACHE, **kw)
    se, sb = e.state_dict(), b.state_dict()
    assert list(se) == list(sb) and "cache_weight" in se and "cache_optimizer_state" in se and "cache_freq" in se
    assert [tuple(v.shape) for v in se.values()] == [tuple(v.shape) for v in sb.values()]
    assert [n for n, _ in e.named_parameters()] == [n for n, _ in b.named_parameters()]
    assert len(e.get_params()) == 4
    with torch.no_grad():
        b.cache_weight.fill_(0.5)
        b.cache_freq.fill_(3)
    e.load_state_dict(b.state_dict())
    assert float(e.cache_weight.detach().min()) == 0.5 and int(e.cache_freq.min()) == 3
    with torch.no_grad():
        e.cache_weight.add_(1.0)
    b.load_state_dict(e.state_dict())
    assert torch.equal(b.cache_weight, e.cache_weight)
    # without the keyword nothing about the class changes
    plain, nocache = emb(ops), bag(ops, use_cache=False)
    assert list(plain.state_dict()) == list(nocache.state_dict()) and not plain.use_cache and plain.cache_weight is None
    assert "cache_weight" not in plain.state_dict() and len(plain.get_params()) == 3


def test_keywords_reach_the_parent(ops):
    m = emb(ops, use_cache=True, cache_size=17, hashtbl_size=64, reference_exact_populate=True, deterministic_cache_update=True)
    assert m.use_cache and m.cache_weight.shape == (17, D_) and m.hashtbl.numel() == 64
    assert m.reference_exact_populate is True and m.deterministic_cache_update is True and m.mode == "sum"
    assert m.prefetch(torch.zeros(3, dtype=torch.int64)) is False and m.prefetch_many([]) is False
    m.reset_cache()
    assert m.warmup


def test_live_module_survives_pickle_and_deepcopy(ops):
    m, hot = live(ops, padding_idx=PAD)
    idx = indices_of((3, 5), hot, seed=6, padded=True)
    want = m(idx).detach()
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert type(other).__name__ == "TTEmbedding" and other.use_cache and not other.warmup and other.padding_idx == PAD
        assert torch.equal(other.cache_state, m.cache_state) and torch.equal(other.cache_weight, m.cache_weight)
        assert torch.equal(other(idx).detach(), want)


def test_empty_input_with_a_live_cache(ops):
    m, _ = live(ops)
    out = m(torch.zeros((4, 0), dtype=torch.int64))
    assert out.shape == (4, 0, D_)
