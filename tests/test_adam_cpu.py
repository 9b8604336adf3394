"""OptimType.EXACT_ADAM without a GPU: the float64 restatement tests/adam_ref.py against torch.optim.Adam / AdamW;
the modules' wiring on the oracle engine (which has no adam_apply: the step then runs the same formula with torch ops) against a
twin module with sparse=False and torch.optim.Adam on its cores; state_dict() keys; the argument errors of ttx_adam_apply; and the
compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_ref as AR
import gen_inputs as G
import oracle_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPS = 0.01, 1e-8
STEPS = 3


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


# ------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("wd", [0.0, 0.05])
@pytest.mark.parametrize("decoupled", [False, True])
def test_restatement_equals_torch_adam_in_float64(wd, decoupled):
    rs = np.random.RandomState(5)
    w0 = rs.randn(7, 13)
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=0.03, betas=(0.8, 0.95), eps=1e-6, weight_decay=wd)
    w, m, v, t = w0, np.zeros_like(w0), np.zeros_like(w0), 0
    for k in range(4):
        g = rs.randn(7, 13) * (10.0 ** (k - 2))
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v, t = AR.step(w, g, m, v, t, 0.03, (0.8, 0.95), 1e-6, wd, decoupled)
        st = opt.state[p]
        np.testing.assert_allclose(w, p.detach().numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-12, atol=0)
        np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-12, atol=0)
        assert t == int(st["step"]) == k + 1


def test_torch_ops_step_equals_the_restatement():
    """the CPU tensors' step (tt_embeddings_ops._adam_apply_torch, fp32) against the float64 restatement: a handful of fp32
    roundings of a step of size ~lr, and of w"""
    import tt_embeddings_ops as ops

    rs = np.random.RandomState(6)
    for wd, dec in ((0.0, False), (0.1, False), (0.1, True)):
        w0, g = rs.randn(301).astype(np.float32), rs.randn(301).astype(np.float32)
        m0, v0 = (0.1 * rs.randn(301)).astype(np.float32), (rs.rand(301) * 0.5).astype(np.float32)
        w, m, v = torch.from_numpy(w0.copy()), torch.from_numpy(m0.copy()), torch.from_numpy(v0.copy())
        step = torch.tensor([7])
        ops._adam_apply_torch([w], [torch.from_numpy(g)], [m], [v], step, 0.05, (0.9, 0.999), 1e-8, wd, dec)
        rw, rm, rv, rt = AR.step(w0, g, m0, v0, 7, 0.05, (0.9, 0.999), 1e-8, wd, dec)
        assert int(step) == rt == 8
        np.testing.assert_allclose(m.numpy(), rm, rtol=0, atol=4e-7)
        np.testing.assert_allclose(v.numpy(), rv, rtol=4e-7, atol=0)
        np.testing.assert_allclose(w.numpy(), rw, rtol=4e-7, atol=0.05 * 2e-6)


# ------------------------------------------------------------------------------------------------------------ the wiring
def _batch(rs, tables, B, E, empty=0.2):
    lens = rs.randint(1, 5, size=tables * B) * (rs.rand(tables * B) > empty)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return torch.from_numpy(rs.randint(0, E, size=int(off[-1])).astype(np.int64)), torch.from_numpy(off)


def _twin(ops, tables, T, seed, **kw):
    p, q, r = G.test_shape(T)
    E, D = int(np.prod(p)), int(np.prod(q))
    mk = lambda **extra: ops.TableBatchedTTEmbeddingBag(tables, E, D, list(r), list(p), list(q), learning_rate=LR, eps=EPS,  # noqa: E731
                                                        weight_dist="uniform", device="cpu", **extra)
    torch.manual_seed(seed)
    a = mk(sparse=True, optimizer=ops.OptimType.EXACT_ADAM, **kw)
    b = mk(sparse=False)
    with torch.no_grad():
        for dst, src in zip(b.tt_cores, a.tt_cores):
            dst.copy_(src)
    return a, b, E, D


def _torch_adam(b_params, kw):
    cls = torch.optim.AdamW if kw.get("decoupled_weight_decay") else torch.optim.Adam
    return cls(b_params, lr=LR, betas=kw.get("betas", (0.9, 0.999)), eps=EPS, weight_decay=kw.get("weight_decay", 0.0))


def _assert_cores_close(a_cores, b_cores, steps, what):
    """fp32 on both sides, the same engine and inputs: what may differ is the rounding of the update itself (torch forms m with a
    lerp and divides where the module multiplies by 1 / sqrt(bc2)) -- some tens of fp32 roundings of a step of size ~lr, bounded
    here by 1e-5 lr per step -- and, from the second step on, the gradient of cores that differ by that much, which Adam's
    normalised step hands on as a relative change of the same order."""
    for t, (x, y) in enumerate(zip(a_cores, b_cores)):
        x, y = x.detach().numpy().astype(np.float64), y.detach().numpy().astype(np.float64)
        tol = steps * 1e-5 * LR + 1e-6 * np.abs(y)
        assert (np.abs(x - y) <= tol).all(), f"{what}: core {t} differs by {np.abs(x - y).max():.3e}"


@pytest.mark.parametrize("T,tables,kw", [(2, 1, {}), (3, 1, {}), (4, 1, {}), (3, 2, {}),
                                         (3, 1, dict(weight_decay=0.05, betas=(0.8, 0.95))),
                                         (3, 2, dict(weight_decay=0.05, decoupled_weight_decay=True))])
def test_three_steps_equal_torch_adam_on_a_dense_twin(ops, T, tables, kw):
    a, b, E, D = _twin(ops, tables, T, 11, **kw)
    opt = _torch_adam(list(b.tt_cores), kw)
    rs = np.random.RandomState(12)
    B = 6
    for k in range(STEPS):
        idx, off = _batch(rs, tables, B, E)
        d_out = torch.from_numpy(rs.randn(tables, B, D).astype(np.float32))
        a(idx, off).backward(d_out)
        opt.zero_grad()
        b(idx, off).backward(d_out)
        opt.step()
        assert all(c.grad is None for c in a.tt_cores), "the fused step leaves no .grad"
        assert int(a.optimizer_step) == k + 1
        _assert_cores_close(a.tt_cores, b.tt_cores, k + 1, f"step {k}")
    for t, c in enumerate(b.tt_cores):  # the moments are torch's
        np.testing.assert_allclose(a.optimizer_state[t].numpy(), opt.state[c]["exp_avg"].numpy(), rtol=1e-4, atol=1e-7 * float(opt.state[c]["exp_avg"].abs().max()))
        np.testing.assert_allclose(a.optimizer_state_v[t].numpy(), opt.state[c]["exp_avg_sq"].numpy(), rtol=1e-4, atol=1e-7 * float(opt.state[c]["exp_avg_sq"].abs().max()))
    # an empty batch: no step, everything bit-identical
    before = {k: v.clone() for k, v in a.state_dict().items()}
    out = a(torch.zeros(0, dtype=torch.int64), torch.zeros(tables * B + 1, dtype=torch.int64))
    out.backward(torch.ones_like(out))
    after = a.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    assert all(c.grad is None for c in a.tt_cores) and int(a.optimizer_step) == STEPS


def test_state_dict_round_trip_continues_the_run(ops):
    a, _, E, D = _twin(ops, 2, 3, 21, weight_decay=0.01)
    rs = np.random.RandomState(22)
    B = 5
    for _ in range(2):
        idx, off = _batch(rs, 2, B, E)
        a(idx, off).backward(torch.from_numpy(rs.randn(2, B, D).astype(np.float32)))
    sd = {k: v.clone() for k, v in a.state_dict().items()}
    assert {"optimizer_step", "optimizer_state.optimizer_state0", "optimizer_state_v.optimizer_state_v2"} <= set(sd)
    assert sd["optimizer_step"].dtype == torch.int64 and tuple(sd["optimizer_step"].shape) == (1,) and int(sd["optimizer_step"]) == 2
    for t in range(3):
        assert sd[f"optimizer_state.optimizer_state{t}"].shape == a.tt_cores[t].shape == sd[f"optimizer_state_v.optimizer_state_v{t}"].shape
    fresh, _, _, _ = _twin(ops, 2, 3, 99, weight_decay=0.01)
    fresh.load_state_dict(sd)
    idx, off = _batch(rs, 2, B, E)
    d_out = torch.from_numpy(rs.randn(2, B, D).astype(np.float32))
    a(idx, off).backward(d_out)
    fresh(idx, off).backward(d_out)
    for k, v in a.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k]), k
    assert int(fresh.optimizer_step) == 3


def test_set_learning_rate_takes_effect_on_the_next_step(ops):
    a, b, E, D = _twin(ops, 1, 3, 31)
    rs = np.random.RandomState(32)
    idx, off = _batch(rs, 1, 6, E)
    d_out = torch.from_numpy(rs.randn(1, 6, D).astype(np.float32))
    a.set_learning_rate(0.0)
    w0 = [c.detach().clone() for c in a.tt_cores]
    a(idx, off).backward(d_out)
    assert all(torch.equal(x, c.detach()) for x, c in zip(w0, a.tt_cores)) and int(a.optimizer_step) == 1
    a.set_learning_rate(LR)
    a(idx, off).backward(d_out)
    assert not any(torch.equal(x, c.detach()) for x, c in zip(w0, a.tt_cores))


def test_unpooled_module(ops):
    p, q, r = G.test_shape(3)
    E, D = int(np.prod(p)), int(np.prod(q))
    mk = lambda **kw: ops.TTEmbedding(E, D, list(r), list(p), list(q), learning_rate=LR, eps=EPS, weight_dist="uniform",  # noqa: E731
                                      device="cpu", padding_idx=3, **kw)
    a, b = mk(optimizer=ops.OptimType.EXACT_ADAM), mk(sparse=False)
    with torch.no_grad():
        for dst, src in zip(b.tt_cores, a.tt_cores):
            dst.copy_(src)
    opt = torch.optim.Adam(list(b.tt_cores), lr=LR, eps=EPS)
    rs = np.random.RandomState(41)
    for k in range(STEPS):
        idx = torch.from_numpy(rs.randint(0, E, size=(4, 5)).astype(np.int64))
        idx[0, :2] = 3
        d_out = torch.from_numpy(rs.randn(4, 5, D).astype(np.float32))
        a(idx).backward(d_out)
        opt.zero_grad()
        b(idx).backward(d_out)
        opt.step()
        assert all(c.grad is None for c in a.tt_cores) and int(a.optimizer_step) == k + 1
        _assert_cores_close(a.tt_cores, b.tt_cores, k + 1, f"step {k}")
    before = [c.detach().clone() for c in a.tt_cores]
    for empty in (torch.zeros((0, 4), dtype=torch.int64), torch.full((2, 3), 3, dtype=torch.int64)):  # no index / padding only
        out = a(empty)
        out.backward(torch.ones_like(out))
        assert int(a.optimizer_step) == STEPS and all(torch.equal(x, c.detach()) for x, c in zip(before, a.tt_cores))
        assert all(c.grad is None for c in a.tt_cores)


def test_mixed_module_steps_every_group_once(ops):
    import ttx_mixed

    D, q, r, B = 12, [2, 3, 2], [4, 5], 7
    Es = [100, 700, 90]
    ps = [[4, 5, 5], [8, 9, 10], [4, 5, 5]]
    mk = lambda **kw: ttx_mixed.MixedTTEmbeddingBag(Es, D, r, ps, q, learning_rate=LR, eps=EPS, weight_dist="uniform",  # noqa: E731
                                                    device="cpu", **kw)
    a, b = mk(optimizer=ops.OptimType.EXACT_ADAM, weight_decay=0.02), mk(sparse=False)
    assert a.group_tables == [[0, 2], [1]]
    b.load_state_dict({k: v for k, v in a.state_dict().items() if "optimizer_st" not in k}, strict=False)
    opt = torch.optim.Adam(list(b.parameters()), lr=LR, eps=EPS, weight_decay=0.02)
    rs = np.random.RandomState(51)
    for k in range(STEPS):
        idx, off = [], []
        for e in Es:
            lens = rs.randint(0, 4, size=B)
            off.append(torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)))
            idx.append(torch.from_numpy(rs.randint(0, e, size=int(lens.sum())).astype(np.int64)))
        ws = [float(x) for x in rs.randn(len(Es))]
        sum((o * w).sum() for o, w in zip(a(idx, off), ws)).backward()
        opt.zero_grad()
        sum((o * w).sum() for o, w in zip(b(idx, off), ws)).backward()
        opt.step()
        for ga, gb in zip(a.groups, b.groups):
            assert int(ga.optimizer_step) == k + 1 and all(c.grad is None for c in ga.tt_cores)
            _assert_cores_close(ga.tt_cores, gb.tt_cores, k + 1, f"step {k}")
    with pytest.raises(NotImplementedError):
        mk(optimizer=ops.OptimType.EXACT_ADAM, fused=True, use_cache=True)


# ------------------------------------------------------------------------------------------------------ unchanged behaviour
SGD_KEYS = ["L", "hashtbl", "cache_state", "tt_cores.0", "tt_cores.1", "tt_cores.2", "optimizer_state.optimizer_state0",
            "optimizer_state.optimizer_state1", "optimizer_state.optimizer_state2"]
CACHED_ADAGRAD_KEYS = ["cache_weight", "L", "hashtbl", "cache_freq", "cache_state", "cache_optimizer_state", "tt_cores.0", "tt_cores.1",
                       "tt_cores.2", "optimizer_state.optimizer_state0", "optimizer_state.optimizer_state1",
                       "optimizer_state.optimizer_state2"]


def test_state_dict_keys_of_the_other_optimizers_are_the_parents(ops):
    """the key lists below were recorded on the commit before EXACT_ADAM existed"""
    p, q, r = G.test_shape(3)
    E, D = int(np.prod(p)), int(np.prod(q))
    mk = lambda cls, *a, **kw: cls(*a, E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu", **kw)  # noqa: E731
    O = ops.OptimType
    for opt in (O.SGD, O.EXACT_ADAGRAD, O.ADAM):
        m = mk(ops.TableBatchedTTEmbeddingBag, 2, optimizer=opt)
        assert list(m.state_dict()) == SGD_KEYS, opt
        assert m.optimizer_state[0].numel() == (0 if opt == O.SGD else m.tt_cores[0].numel())
        assert list(mk(ops.TTEmbedding, optimizer=opt).state_dict()) == SGD_KEYS
    m = mk(ops.TTEmbeddingBag, optimizer=O.EXACT_ADAGRAD, use_cache=True, cache_size=8, hashtbl_size=64)
    assert list(m.state_dict()) == CACHED_ADAGRAD_KEYS
    # EXACT_ADAM without sparse: the optimizer is ignored, no state exists
    m = mk(ops.TableBatchedTTEmbeddingBag, 2, optimizer=O.EXACT_ADAM, sparse=False)
    assert list(m.state_dict()) == SGD_KEYS and all(s.numel() == 0 for s in m.optimizer_state) and m._adam is None
    import ttx_dense as TD

    mk_d = lambda **kw: TD.DenseTableBatchedEmbeddingBag([3, 4], 8, device="cpu", **kw)  # noqa: E731
    assert list(mk_d().state_dict()) == ["weight", "optimizer_state"] == list(mk_d(optimizer=O.EXACT_ADAGRAD).state_dict())
    assert list(mk_d(optimizer=O.EXACT_ADAM, sparse=False).state_dict()) == ["weight", "optimizer_state"]
    d = mk_d(optimizer=O.EXACT_ADAM)
    assert list(d.state_dict()) == ["weight", "optimizer_state", "optimizer_state_v", "optimizer_step"]
    assert tuple(d.optimizer_state.shape) == tuple(d.optimizer_state_v.shape) == (7, 8) and d.optimizer_step.dtype == torch.int64
    d.optimizer_state.fill_(1.0), d.optimizer_state_v.fill_(2.0), d.optimizer_step.fill_(5)
    d.reset_parameters()
    assert not d.optimizer_state.any() and not d.optimizer_state_v.any() and int(d.optimizer_step) == 0


def test_limits_are_refused_at_construction(ops):
    p, q, r = G.test_shape(3)
    E, D = int(np.prod(p)), int(np.prod(q))
    A = ops.OptimType.EXACT_ADAM
    kw = dict(tt_p_shapes=list(p), tt_q_shapes=list(q), weight_dist="uniform", device="cpu", optimizer=A)
    with pytest.raises(NotImplementedError):
        ops.TableBatchedTTEmbeddingBag(2, E, D, list(r), use_cache=True, cache_size=8, hashtbl_size=64, **kw)
    with pytest.raises(NotImplementedError):
        ops.TTEmbeddingBag(E, D, list(r), use_cache=True, cache_size=8, hashtbl_size=64, **kw)
    with pytest.raises(NotImplementedError):
        ops.TTEmbedding(E, D, list(r), use_cache=True, cache_size=8, hashtbl_size=64, **kw)
    import ttx_mixed

    with pytest.raises(NotImplementedError):
        ttx_mixed.VarTableTTEmbeddingBag([E, E - 1], D, list(r), [list(p), list(p)], list(q), optimizer=A, weight_dist="uniform",
                                         device="cpu", use_cache=True, cache_size=8, hashtbl_size=64)
    for bad in (dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            ops.TTEmbeddingBag(E, D, list(r), use_cache=False, **kw, **bad)
    # the keywords are read under EXACT_ADAM only
    ops.TTEmbeddingBag(E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu", use_cache=False, betas=(7.0, 7.0))
    assert ops.OptimType.EXACT_ADAM.value == "exact_adam" and ops.OptimType.ADAM.value == "adam"


def test_sparse_false_leaves_gradients_and_adam_member_is_still_adagrad(ops):
    a, b, E, D = _twin(ops, 1, 3, 61)
    rs = np.random.RandomState(62)
    idx, off = _batch(rs, 1, 6, E)
    d_out = torch.from_numpy(rs.randn(1, 6, D).astype(np.float32))
    p, q, r = G.test_shape(3)
    m = ops.TableBatchedTTEmbeddingBag(1, E, D, list(r), list(p), list(q), optimizer=ops.OptimType.EXACT_ADAM, sparse=False,
                                       weight_dist="uniform", device="cpu")
    w0 = [c.detach().clone() for c in m.tt_cores]
    m(idx, off).backward(d_out)
    assert all(c.grad is not None and c.grad.abs().sum() > 0 for c in m.tt_cores)
    assert all(torch.equal(x, c.detach()) for x, c in zip(w0, m.tt_cores)) and not hasattr(m, "optimizer_step")
    # OptimType.ADAM keeps the reference's behaviour: the Adagrad kernel, its state in optimizer_state
    torch.manual_seed(3)
    ad = ops.TableBatchedTTEmbeddingBag(1, E, D, list(r), list(p), list(q), optimizer=ops.OptimType.ADAM, learning_rate=LR,
                                        eps=EPS, weight_dist="uniform", device="cpu")
    torch.manual_seed(3)
    ag = ops.TableBatchedTTEmbeddingBag(1, E, D, list(r), list(p), list(q), optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=LR,
                                        eps=EPS, weight_dist="uniform", device="cpu")
    ad(idx, off).backward(d_out)
    ag(idx, off).backward(d_out)
    assert not hasattr(ad, "optimizer_state_v") and ad._adam is None
    for t in range(3):
        assert torch.equal(ad.tt_cores[t].detach(), ag.tt_cores[t].detach()) and torch.equal(ad.optimizer_state[t], ag.optimizer_state[t])
        assert float(ad.optimizer_state[t].sum()) > 0  # (sum of g^2: Adagrad's accumulator)


# --------------------------------------------------------------------------------------------------------------- the ABI
i32, i64, f32, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t


def _libs():
    for name in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", name))
        lib.ttx_last_error.restype = ctypes.c_char_p
        lib.ttx_adam_apply_workspace_bytes.restype = sz
        lib.ttx_adam_apply_workspace_bytes.argtypes = [i32]
        lib.ttx_adam_apply.argtypes = [i32, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, i32, vp, sz, vp]
        yield lib


def test_entry_points_are_declared_and_the_shim_has_the_call():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+ttx_adam_apply\s*\(", hdr) and re.search(r"\bsize_t\s+ttx_adam_apply_workspace_bytes\s*\(", hdr)
    import tt_embeddings as E

    assert callable(E.adam_apply) and E.ADAM_MAX_TENSORS == 16
    z = torch.zeros(4)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine)
        E.adam_apply([z], [z], [z], [z], torch.zeros(1, dtype=torch.int64), 0.1, (0.9, 0.999), 1e-8)


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced; this machine has no GPU: a call that reached the runtime would return -4)"""
    fake, odd, odd8 = 4096, 4098, 4100
    for lib in _libs():
        need = lib.ttx_adam_apply_workspace_bytes(2)
        assert need > 0

        def call(**kw):
            a = dict(n=2, numel=(i64 * 2)(8, 5), w=(vp * 2)(fake, fake), g=(vp * 2)(fake, fake), m=(vp * 2)(fake, fake),
                     v=(vp * 2)(fake, fake), step=fake, lr=0.1, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, dec=0, ws=fake, wsb=need)
            a.update(kw)
            return lib.ttx_adam_apply(a["n"], a["numel"], a["w"], a["g"], a["m"], a["v"], a["step"], a["lr"], a["b1"], a["b2"],
                                      a["eps"], a["wd"], a["dec"], a["ws"], a["wsb"], None)

        bad = [dict(n=-1), dict(n=17), dict(numel=(i64 * 2)(8, -5)), dict(numel=None), dict(w=None), dict(g=None), dict(m=None),
               dict(v=None), dict(w=(vp * 2)(fake, None)), dict(g=(vp * 2)(None, fake)), dict(m=(vp * 2)(fake, 0)),
               dict(v=(vp * 2)(0, fake)), dict(w=(vp * 2)(fake, odd)), dict(g=(vp * 2)(odd, fake)), dict(m=(vp * 2)(fake, odd)),
               dict(v=(vp * 2)(odd, fake)), dict(step=None), dict(step=odd), dict(step=odd8), dict(b1=1.0), dict(b1=-0.1),
               dict(b2=1.0), dict(b2=-1e-3), dict(b1=float("nan")), dict(eps=-1e-8), dict(ws=None), dict(wsb=need - 1), dict(wsb=0)]
        for kw in bad:
            assert call(**kw) == -1, kw
            assert b"adam_apply" in lib.ttx_last_error(), lib.ttx_last_error()
        # nothing to do: 0, nothing launched, step and workspace not needed -- a zero-size tensor may have NULL pointers
        assert call(n=0, numel=None, w=None, g=None, m=None, v=None, step=None, ws=None, wsb=0) == 0
        assert call(numel=(i64 * 2)(0, 0), w=(vp * 2)(None, None), step=None, ws=None, wsb=0) == 0


# --------------------------------------------------------------------------------------------------- the compiler report
def test_adam_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed); the figures are in DESIGN.md 4.17"""
    from test_kernel_resources import resources

    res = resources("ttx_adam.hip")
    names = sorted(k for k in res if "adam_" in k)
    for w in ("adam_step_kernel", "adam_apply_kernelILi0", "adam_apply_kernelILi1", "adam_apply_kernelILi2"):
        assert sum(w in k for k in names) == 1, (w, names)
    assert len(names) == 4, names
    for k in names:
        print(k, res[k])
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["VGPRs"] <= 64 and res[k]["Occupancy"] >= 8, (k, res[k])
        assert res[k]["LDS Size"] <= 6 * 16 * 8, (k, res[k])  # (the staged pointers, sizes and first chunks: nothing else)
