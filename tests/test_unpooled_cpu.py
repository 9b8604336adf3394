"""CPU tests (no GPU) of the unpooled lookup `TTEmbedding` (nn.Embedding on a TT table): on top of the oracle engine the module
against torch's own F.embedding on the expanded table and against the float64 reference (forward, dense core gradients, one
fused SGD / Adagrad step), its state / pickling / keyword behaviour, empty input, and the C ABI of ttx_rows_expand /
ttx_rows_collect (declared, exported, argument checks)."""
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
import tt_ref64 as R64
from test_padding_idx_cpu import D_, E_, P, PAD, Q, R
from util import EPS, LR, assert_adagrad_close, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(), (7,), (3, 5), (2, 3, 4)]


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
    return ops.TTEmbeddingBag(E_, D_, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", **kw)


def indices_of(shape, seed=1, padded=False):
    """int64 indices of `shape`; padded: about a third of them PAD (the 0-D input: PAD itself), none by accident otherwise"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, E_, size=shape).astype(np.int64)
    idx = np.where(idx == PAD, PAD + 1, idx)
    if padded:
        idx = np.where(rs.rand(*shape) < 0.35, PAD, idx) if shape else np.array(PAD, np.int64)
        if idx.ndim >= 1 and idx.size > 2:
            idx.reshape(-1)[0], idx.reshape(-1)[1] = PAD, PAD + 2  # (at least one of each)
    return torch.from_numpy(np.asarray(idx, dtype=np.int64))


# ----------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_forward_equals_torch_embedding_on_the_expanded_table(ops, shape, dtype):
    m = emb(ops)
    idx = indices_of(shape)
    out = m(idx.to(dtype))
    assert out.shape == shape + (D_,) and out.dtype == torch.float32
    assert_close(out.detach().numpy(), F.embedding(idx, m.full_weight()).detach().numpy(), f"forward {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
def test_padded_forward_equals_torch_embedding_on_the_table_with_that_row_zeroed(ops, shape, dtype):
    m = emb(ops, padding_idx=PAD)
    idx = indices_of(shape, padded=True)
    w0 = m.full_weight().detach().clone()
    w0[PAD] = 0
    out = m(idx.to(dtype))
    assert out.shape == shape + (D_,)
    assert_close(out.detach().numpy(), F.embedding(idx, w0).numpy(), f"padded forward {shape}")
    assert (idx == PAD).any()
    assert (out.detach()[idx == PAD] == 0).all(), "padding positions are exact zeros"
    assert_close(out.detach().numpy(), F.embedding(idx, m.full_weight().detach(), padding_idx=PAD).numpy() * (idx != PAD).numpy()[..., None],
                 "padded forward vs torch's own rows")


# --------------------------------------------------------------------------------------------------- gradients vs float64
def reference(m, idx, d_out, pad):
    """tt_ref64 on the live positions, one bag each -> (dict, live indices, keep mask)"""
    flat = idx.reshape(-1).numpy()
    keep = flat != pad if pad is not None else np.ones(flat.size, bool)
    live = flat[keep]
    cores = [c.detach().numpy().copy() for c in m.tt_cores]
    d = d_out.reshape(-1, D_).numpy()[keep]
    ref = R64.forward_backward(1, P, Q, R, live.size, live, np.arange(live.size), np.zeros(live.size, np.int64), cores,
                               d_out=d[None])
    return ref, cores, keep


@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_dense_core_gradients_vs_float64(ops, pad):
    m = emb(ops, padding_idx=pad)
    idx = indices_of((3, 5), seed=2, padded=pad is not None)
    d_out = torch.from_numpy(np.random.RandomState(4).standard_normal((3, 5, D_)).astype(np.float32))
    ref, _, keep = reference(m, idx, d_out, pad)
    out = m(idx)
    assert_close(out.detach().reshape(-1, D_).numpy()[keep], ref["out"][0], "forward vs float64")
    out.backward(d_out)
    for k in range(3):
        assert_close(m.tt_cores[k].grad.numpy(), ref["grads"][k], f"grad{k} vs float64")


@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_fused_sgd_step_vs_float64(ops, pad):
    m = emb(ops, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=pad)
    idx = indices_of((3, 5), seed=5, padded=pad is not None)
    d_out = torch.from_numpy(np.random.RandomState(6).standard_normal((3, 5, D_)).astype(np.float32))
    ref, cores, _ = reference(m, idx, d_out, pad)
    m(idx).backward(d_out)
    want = R64.sgd_step(cores, ref["grads"], LR)
    for k in range(3):
        assert m.tt_cores[k].grad is None
        assert_close(m.tt_cores[k].detach().numpy(), want[k], f"sgd core{k} vs float64")


@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_fused_adagrad_step_vs_float64(ops, pad):
    m = emb(ops, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=LR, eps=EPS, padding_idx=pad)
    idx = indices_of((3, 5), seed=7, padded=pad is not None)
    d_out = torch.from_numpy(np.random.RandomState(8).standard_normal((3, 5, D_)).astype(np.float32))
    ref, cores, _ = reference(m, idx, d_out, pad)
    state0 = [np.zeros_like(c) for c in cores]
    m(idx).backward(d_out)
    e_w, e_s = R64.adagrad_step(cores, state0, ref["grads"], ref["touched"], LR, EPS)
    for k in range(3):
        R64.assert_state_close(m.optimizer_state[k].numpy(), e_s[k], ref["grads"][k], f"adagrad state{k} vs float64")
        assert_adagrad_close(m.tt_cores[k].detach().numpy(), e_w[k], ref["grads"][k], f"adagrad core{k} vs float64", lr=LR, eps=EPS)


def test_padding_positions_receive_no_gradient(ops):
    """a batch of PAD and one other index: the dense gradients are those of the one live lookup"""
    a, b = emb(ops, padding_idx=PAD), emb(ops)
    idx = torch.tensor([[PAD, 17, PAD]])
    d = torch.from_numpy(np.random.RandomState(9).standard_normal((1, 3, D_)).astype(np.float32))
    a(idx).backward(d)
    b(torch.tensor([17])).backward(d[:, 1])
    for k in range(3):
        assert torch.equal(a.tt_cores[k].grad, b.tt_cores[k].grad)


# ------------------------------------------------------------------------------------------------------ state and pickling
def test_state_dict_is_the_bag_modules_and_loads_both_ways(ops):
    e, b = emb(ops, padding_idx=PAD, optimizer=ops.OptimType.EXACT_ADAGRAD, sparse=True), \
        bag(ops, optimizer=ops.OptimType.EXACT_ADAGRAD, sparse=True)
    se, sb = e.state_dict(), b.state_dict()
    assert list(se) == list(sb)
    assert [tuple(v.shape) for v in se.values()] == [tuple(v.shape) for v in sb.values()]
    with torch.no_grad():
        for c in b.tt_cores:
            c.mul_(1.5)
        b.optimizer_state[1].fill_(0.25)
    e.load_state_dict(b.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(e.tt_cores, b.tt_cores)) and float(e.optimizer_state[1].min()) == 0.25
    with torch.no_grad():
        for c in e.tt_cores:
            c.add_(1.0)
    b.load_state_dict(e.state_dict())
    assert all(torch.equal(x, y) for x, y in zip(e.tt_cores, b.tt_cores))
    # the same table: an unpooled lookup is the bag module's one-lookup bags
    idx = indices_of((7,), seed=3)
    e2 = emb(ops, optimizer=ops.OptimType.EXACT_ADAGRAD)
    e2.load_state_dict(b.state_dict())
    with torch.no_grad():
        assert torch.equal(e2(idx), b(idx, torch.arange(8)))
    assert torch.equal(e2.full_weight(), b.full_weight())
    e2.set_learning_rate(0.5)
    assert e2.learning_rate == 0.5 and len(e2.get_params()) == 3
    e2.reset_parameters("uniform")


def test_padding_idx_survives_pickle_and_deepcopy(ops):
    m = emb(ops, padding_idx=-3)
    assert m.padding_idx == E_ - 3
    idx = indices_of((3, 5), seed=4)
    for other in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert type(other).__name__ == "TTEmbedding" and other.padding_idx == E_ - 3
        assert torch.equal(other(idx), m(idx))
    m(idx)  # (the cached offsets of the one-lookup bags are not state)
    assert pickle.loads(pickle.dumps(m)).padding_idx == E_ - 3


def test_padding_idx_keyword_follows_torch(ops):
    assert emb(ops).padding_idx is None
    assert emb(ops, padding_idx=None).padding_idx is None
    assert emb(ops, padding_idx=0).padding_idx == 0
    assert emb(ops, padding_idx=E_ - 1).padding_idx == E_ - 1
    assert emb(ops, padding_idx=-1).padding_idx == E_ - 1
    assert emb(ops, padding_idx=-E_).padding_idx == 0
    assert emb(ops, padding_idx=np.int64(7)).padding_idx == 7
    for bad in (E_, -E_ - 1, 1.5, "3", True):
        with pytest.raises(ValueError):
            emb(ops, padding_idx=bad)
    assert torch.nn.Embedding(E_, 4, padding_idx=-1).padding_idx == E_ - 1
    with pytest.raises(AssertionError):
        torch.nn.Embedding(E_, 4, padding_idx=E_)


def test_call_form(ops):
    m = emb(ops)
    with pytest.raises(ValueError):
        m(torch.zeros(3))  # float indices
    assert m.prefetch(torch.zeros(3, dtype=torch.int64)) is False and m.prefetch_many([]) is False
    assert not m.use_cache and m.num_tables == 1


# ------------------------------------------------------------------------------------------------------------- empty input
@pytest.mark.parametrize("shape", [(0,), (4, 0), (0, 3)], ids=str)
@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_empty_input(ops, shape, pad):
    idx = torch.zeros(shape, dtype=torch.int64)
    m = emb(ops, padding_idx=pad)
    out = m(idx)
    assert out.shape == shape + (D_,) and out.dtype == torch.float32
    out.backward(torch.zeros_like(out))
    for c in m.tt_cores:
        assert c.grad is not None and c.grad.shape == c.shape and not c.grad.any(), "sparse=False: zero gradients"
    f = emb(ops, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, padding_idx=pad)
    before = [c.detach().clone() for c in f.tt_cores]
    out = f(idx)
    assert out.shape == shape + (D_,)
    out.backward(torch.zeros_like(out))
    assert all(torch.equal(a, b) for a, b in zip(before, f.tt_cores)) and all(not s.any() for s in f.optimizer_state)


def test_all_padding_input(ops):
    idx = torch.full((2, 3), PAD, dtype=torch.int64)
    m = emb(ops, padding_idx=PAD)
    out = m(idx)
    assert out.shape == (2, 3, D_) and not out.any()
    out.backward(torch.ones_like(out))
    assert all(c.grad is not None and not c.grad.any() for c in m.tt_cores)
    f = emb(ops, sparse=True, padding_idx=PAD)
    before = [c.detach().clone() for c in f.tt_cores]
    f(idx).backward(torch.ones(2, 3, D_))
    assert all(torch.equal(a, b) for a, b in zip(before, f.tt_cores))


# ----------------------------------------------------------------------------------------------------------------- the ABI
def test_rows_entry_points_are_declared_and_exported_and_check_their_arguments():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    for name in ("ttx_rows_expand", "ttx_rows_collect"):
        assert re.search(r"\bint\s+%s\s*\(\s*int64_t n,\s*int32_t D,\s*const int64_t\*\s*rank," % name, hdr), \
            f"{name} is not declared in include/ttx.h"
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        for name in ("ttx_rows_expand", "ttx_rows_collect"):
            f = getattr(lib, name)
            f.argtypes = [i64, i32, vp, vp, vp, vp]
            # nothing to move: 0, and nothing touches a device (no buffers at all)
            assert f(0, 4, None, None, None, None) == 0
            # bad arguments: -1 with a message, before anything is launched (the pointers below are never dereferenced)
            fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)
            for args in ((-1, 4, fake, fake, fake, None),        # negative n
                         (8, 0, fake, fake, fake, None),         # D == 0
                         (8, -4, fake, fake, fake, None),        # negative D
                         (1 << 31, 4, fake, fake, fake, None),   # n >= 2^31
                         (8, 4, None, fake, fake, None),         # NULL rank
                         (8, 4, fake, None, fake, None),         # NULL source
                         (8, 4, fake, fake, None, None),         # NULL destination
                         (8, 4, fake, odd, fake, None),          # source not 4-byte aligned
                         (8, 4, fake, fake, odd, None)):         # destination not 4-byte aligned
                assert f(*args) == -1, (name, args)
                assert name[4:].encode() in lib.ttx_last_error(), lib.ttx_last_error()


def test_engine_exposes_the_rows_calls_and_the_plan_count():
    import inspect

    import tt_embeddings as E

    assert callable(E.rows_expand) and callable(E.rows_collect)
    sig = inspect.signature(E.make_plan)
    assert list(sig.parameters)[-1] == "n_dev" and sig.parameters["n_dev"].default is None
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.rows_expand(torch.zeros(5, dtype=torch.int64), torch.zeros(4, 8))
    with pytest.raises(RuntimeError):
        E.rows_collect(torch.zeros(5, dtype=torch.int64), torch.zeros(4, 8))


def test_rows_kernels_use_no_scratch_and_no_lds():
    """the compiler's own resource report for gfx950 (no GPU needed)"""
    from test_kernel_resources import resources

    res = resources("ttx_rows.hip")
    names = sorted(k for k in res if "rows_" in k)
    assert len(names) == 4 and all(any(w in k for k in names) for w in
                                   ("rows_expand4_kernel", "rows_expand1_kernel", "rows_collect4_kernel", "rows_collect1_kernel")), names
    for k in names:
        assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs"] <= 64, (k, res[k])
        assert res[k].get("LDS Size", res[k].get("LDSSize", 0)) == 0, (k, res[k])
