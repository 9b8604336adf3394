"""CPU tests (no GPU) of the dense member tables: the float64 restatement tests/dense_ref.py against torch's own F.embedding_bag,
autograd and optimizers; the argument checks of the C ABI (every error before anything touches a device); the selection helper
of MixedTTEmbeddingBag(dense_below=, dense=); and the compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dense_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ES = [3, 1, 24, 1460]
B_, D_ = 7, 6
PADS = [2, None, 5, 0]
BASE = np.concatenate([[0], np.cumsum(ES)]).astype(np.int64)


def weights(seed=0):
    return np.random.RandomState(seed).uniform(-1, 1, size=(int(BASE[-1]), D_))


def torch_tables(w, indices, offsets, mode, pads, psw):
    """one F.embedding_bag per table on float64 leaves -> (leaves, out [tables * B, D])"""
    leaves, outs = [], []
    for t in range(len(ES)):
        leaf = torch.tensor(w[BASE[t]:BASE[t + 1]], dtype=torch.float64, requires_grad=True)
        s, e = int(offsets[t * B_]), int(offsets[(t + 1) * B_])
        off = torch.from_numpy(offsets[t * B_:(t + 1) * B_ + 1] - s)
        pw = None if psw is None else torch.from_numpy(psw[s:e].astype(np.float64))
        outs.append(F.embedding_bag(torch.from_numpy(indices[s:e]), leaf, off, mode=mode, per_sample_weights=pw,
                                    include_last_offset=True, padding_idx=None if pads is None else pads[t]))
        leaves.append(leaf)
    return leaves, torch.cat(outs)


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_reference_forward_and_gradient_equal_torch(mode, padded):
    pads = PADS if padded else None
    idx, off, psw = DR.make_batch(3, ES, B_, pad=pads, tie_table=2)
    psw = psw if mode == "sum" else None
    w = weights()
    if mode == "max":  # a tie inside a bag: the bag's first two slots hold the same row
        s = int(off[2 * B_])
        assert idx[s] == idx[s + 1]
    lens = np.diff(off)
    assert (lens == 0).sum() >= len(lens) // 5, "a fifth of the bags are empty"
    out, live, arg = DR.forward(w, idx, off, BASE, B_, mode, pads, psw)
    leaves, t_out = torch_tables(w, idx, off, mode, pads, psw)
    np.testing.assert_allclose(out, t_out.detach().numpy(), rtol=1e-12, atol=1e-14)
    if padded:
        assert live[1] == 0 and not out[1].any(), "a bag of padding only is zero"
    d_out = np.random.RandomState(5).standard_normal(out.shape)
    t_out.backward(torch.from_numpy(d_out))
    G, touched, _ = DR.row_grads(w, idx, off, BASE, B_, d_out, mode, pads, psw)
    for t in range(len(ES)):
        np.testing.assert_allclose(G[BASE[t]:BASE[t + 1]], leaves[t].grad.numpy(), rtol=1e-12, atol=1e-14)
    assert not G[~touched].any()
    if mode == "mean" and padded:  # the divisor is the live count, not the bag's length: the case holds such a bag
        assert ((live > 0) & (live < lens)).any()


def test_reference_weight_gradient_equals_torch():
    idx, off, psw = DR.make_batch(4, ES, B_, pad=PADS)
    w = weights(1)
    d_out = np.random.RandomState(6).standard_normal((len(off) - 1, D_))
    pw = torch.tensor(psw.astype(np.float64), requires_grad=True)
    outs = []
    for t in range(len(ES)):
        s, e = int(off[t * B_]), int(off[(t + 1) * B_])
        outs.append(F.embedding_bag(torch.from_numpy(idx[s:e]), torch.from_numpy(w[BASE[t]:BASE[t + 1]]),
                                    torch.from_numpy(off[t * B_:(t + 1) * B_ + 1] - s), mode="sum", per_sample_weights=pw[s:e],
                                    include_last_offset=True, padding_idx=PADS[t]))
    torch.cat(outs).backward(torch.from_numpy(d_out))
    _, _, d_psw = DR.row_grads(w, idx, off, BASE, B_, d_out, "sum", PADS, psw)
    np.testing.assert_allclose(d_psw, pw.grad.numpy(), rtol=1e-12, atol=1e-14)
    bag, row = DR.lookups(idx, off, BASE, B_, PADS)
    assert (row < 0).any() and not d_psw[row < 0].any(), "0 at padding"


@pytest.mark.parametrize("opt", ["sgd", "adagrad"])
def test_reference_three_steps_equal_torch_optimizers(opt):
    lr, eps = 0.1, 1e-10
    w = weights(2)
    leaves = [torch.tensor(w[BASE[t]:BASE[t + 1]], dtype=torch.float64, requires_grad=True) for t in range(len(ES))]
    o = torch.optim.SGD(leaves, lr=lr) if opt == "sgd" else torch.optim.Adagrad(leaves, lr=lr, eps=eps)
    state = np.zeros_like(w)
    for step in range(3):
        idx, off, _ = DR.make_batch(10 + step, ES, B_, pad=PADS)
        d_out = np.random.RandomState(20 + step).standard_normal((len(off) - 1, D_))
        G, touched, _ = DR.row_grads(w, idx, off, BASE, B_, d_out, "sum", PADS)
        if opt == "sgd":
            w = DR.sgd(w, G, touched, lr)
        else:
            w, state = DR.adagrad(w, state, G, touched, lr, eps)
        o.zero_grad()
        outs = []
        for t in range(len(ES)):
            s, e = int(off[t * B_]), int(off[(t + 1) * B_])
            outs.append(F.embedding_bag(torch.from_numpy(idx[s:e]), leaves[t], torch.from_numpy(off[t * B_:(t + 1) * B_ + 1] - s),
                                        mode="sum", include_last_offset=True, padding_idx=PADS[t]))
        torch.cat(outs).backward(torch.from_numpy(d_out))
        o.step()
        for t in range(len(ES)):
            np.testing.assert_allclose(w[BASE[t]:BASE[t + 1]], leaves[t].detach().numpy(), rtol=1e-11, atol=1e-13,
                                       err_msg=f"{opt} step {step} table {t}")


def test_reference_rowwise_adagrad_by_hand():
    w, s = np.array([[1.0, 2.0], [3.0, 4.0]]), np.array([0.5, 0.25])
    G, touched = np.array([[3.0, 4.0], [0.0, 0.0]]), np.array([True, False])
    w1, s1 = DR.rowwise_adagrad(w, s, G, touched, 0.1, 1e-3)
    assert s1[0] == 0.5 + 12.5 and s1[1] == 0.25
    np.testing.assert_allclose(w1[0], w[0] - 0.1 * G[0] / (np.sqrt(13.0) + 1e-3), rtol=1e-15)
    assert (w1[1] == w[1]).all()


def test_reference_clamps_bad_indices_into_their_table():
    bag, row = DR.lookups(np.array([5, -7, 99]), np.array([0, 1, 2, 3]), np.array([0, 3, 4, 28]), 1)
    assert row.tolist() == [2, -1, 27]


# ----------------------------------------------------------------------------------------------------------------- the ABI
i64, i32, vp, f32, sz = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p, ctypes.c_float, ctypes.c_size_t


def _libs():
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        lib.ttx_dense_bags_forward.argtypes = [i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
        lib.ttx_dense_bags_backward_workspace_bytes.restype = sz
        lib.ttx_dense_bags_backward_workspace_bytes.argtypes = [i64, i64, i32]
        lib.ttx_dense_bags_backward.argtypes = [i32, i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, f32, i32, vp, vp,
                                                vp, vp, vp, sz, vp]
        lib.ttx_dense_bags_info.argtypes = [i32, i64, ctypes.POINTER(i32)]
        yield lib


def test_entry_points_are_declared():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    for name in ("ttx_dense_bags_forward", "ttx_dense_bags_backward", "ttx_dense_bags_info"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), f"{name} is not declared in include/ttx.h"
    assert re.search(r"\bsize_t\s+ttx_dense_bags_backward_workspace_bytes\s*\(", hdr)


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced; this machine has no GPU: a call that reached the runtime would return -4)"""
    fake, odd = 4096, 4098
    base = (i64 * 3)(0, 3, 27)
    pad = (i64 * 2)(-1, 4)
    for lib in _libs():
        def fwd(**kw):
            a = dict(nt=2, B=4, D=8, nnz=16, idx=fake, off=fake, base=base, pad=None, psw=None, mode=0, w=fake, out=fake,
                     live=None, arg=None)
            a.update(kw)
            return lib.ttx_dense_bags_forward(a["nt"], a["B"], a["D"], a["nnz"], a["idx"], a["off"], a["base"], a["pad"], a["psw"],
                                              a["mode"], a["w"], a["out"], a["live"], a["arg"], None)

        def bwd(**kw):
            a = dict(optim=0, nt=2, B=4, D=8, nnz=16, idx=fake, off=fake, base=base, pad=None, psw=None, mode=0, live=None,
                     arg=None, g=fake, width=0, state=None, w=fake, dw=None, dpsw=None, ws=fake, wsb=1 << 30)
            a.update(kw)
            return lib.ttx_dense_bags_backward(a["optim"], a["nt"], a["B"], a["D"], a["nnz"], a["idx"], a["off"], a["base"],
                                               a["pad"], a["psw"], a["mode"], a["live"], a["arg"], a["g"], 0.1, 1e-8, a["width"],
                                               a["state"], a["w"], a["dw"], a["dpsw"], a["ws"], a["wsb"], None)

        shared = [dict(B=-1), dict(nnz=-1), dict(nnz=1 << 31), dict(B=1 << 30), dict(nt=0), dict(nt=65), dict(base=None),
                  dict(base=(i64 * 3)(1, 3, 27)), dict(base=(i64 * 3)(0, 3, 3)), dict(base=(i64 * 3)(0, 5, 4)), dict(D=0), dict(D=-8),
                  dict(psw=fake, mode=1), dict(psw=fake, mode=2), dict(mode=3), dict(mode=1), dict(mode=2), dict(idx=None),
                  dict(off=None), dict(idx=odd), dict(off=odd), dict(psw=odd), dict(w=None), dict(w=odd)]
        for kw in shared + [dict(out=None), dict(out=odd), dict(mode=1, live=odd), dict(mode=2, arg=odd)]:
            assert fwd(**kw) == -1, ("forward", kw)
            assert b"dense_bags_forward" in lib.ttx_last_error(), lib.ttx_last_error()
        more = [dict(optim=3), dict(optim=-1), dict(width=1), dict(width=8), dict(optim=1, width=0, state=fake),
                dict(optim=1, width=4, state=fake), dict(optim=1, width=8, state=None), dict(optim=1, width=1, state=odd),
                dict(optim=2, width=1, dw=fake), dict(optim=2, dw=None), dict(optim=2, dw=odd), dict(g=None), dict(g=odd),
                dict(mode=1, live=odd), dict(mode=2, arg=odd), dict(dpsw=odd), dict(dpsw=fake, mode=1, live=fake),
                dict(dpsw=fake, optim=2, dw=fake, w=None)]
        for kw in shared + more:
            if kw in (dict(w=None), dict(w=odd)):
                kw = dict(kw, optim=0)
            assert bwd(**kw) == -1, ("backward", kw)
            assert b"dense_bags_backward" in lib.ttx_last_error(), lib.ttx_last_error()
        need = lib.ttx_dense_bags_backward_workspace_bytes(8, 16, 8)
        assert need > 0
        for kw in (dict(wsb=need - 1), dict(ws=None), dict(wsb=0)):
            assert bwd(**kw) == -2, ("workspace", kw)  # TTX_EWORKSPACE
            assert b"workspace" in lib.ttx_last_error()
        # a padding array is read, not refused; per-table padding given misaligned is
        assert fwd(pad=ctypes.cast(ctypes.addressof(pad) + 4, vp)) == -1
        out = (i32 * 2)()
        assert lib.ttx_dense_bags_info(64, 1000, out) == 0 and out[0] > 0 and out[1] >= 0
        assert lib.ttx_dense_bags_info(0, 1000, out) == -1 and lib.ttx_dense_bags_info(64, 10, None) == -1


def test_engine_exposes_the_dense_calls():
    import tt_embeddings as E

    assert callable(E.dense_bags_forward) and callable(E.dense_bags_backward)
    info = E.dense_bags_info(64, 1000)
    assert info["split"] > 0 and set(info) == {"split", "one_launch"}
    with pytest.raises(RuntimeError):  # (no CPU path in the engine)
        E.dense_bags_forward(torch.zeros(4, dtype=torch.int64), torch.arange(5), [0, 3], torch.zeros(3, 8))


def test_module_refuses_cpu_tensors_and_bad_keywords():
    import ttx_dense as TD

    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, mode="min", device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, padding_idx=[1], device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3, 4], 8, padding_idx=[3, None], device="cpu")
    with pytest.raises(ValueError):
        TD.DenseTableBatchedEmbeddingBag([3] * 65, 8, device="cpu")
    m = TD.DenseTableBatchedEmbeddingBag(ES, D_, optimizer=TD.OptimType.EXACT_ROWWISE_ADAGRAD, padding_idx=[-1, None, 5, 0], device="cpu")
    assert m.padding_idx == [2, None, 5, 0] and m.row_base == BASE.tolist()
    assert tuple(m.weight.shape) == (int(BASE[-1]), D_) and tuple(m.optimizer_state.shape) == (int(BASE[-1]),)
    assert list(m.state_dict()) == ["weight", "optimizer_state"]
    for k, e in enumerate(ES):
        tw = m.table_weight(k)
        assert tuple(tw.shape) == (e, D_) and float(tw.abs().max()) <= 1.0 / np.sqrt(e)
        assert tw.data_ptr() == m.weight.data_ptr() + int(BASE[k]) * D_ * 4, "a view"
    assert TD.DenseTableBatchedEmbeddingBag(ES, D_, device="cpu").optimizer_state.numel() == 0
    assert tuple(TD.DenseTableBatchedEmbeddingBag(ES, D_, optimizer=TD.OptimType.EXACT_ADAGRAD, device="cpu").optimizer_state.shape) \
        == (int(BASE[-1]), D_)
    with pytest.raises(RuntimeError):
        m(torch.zeros(8, dtype=torch.int64), torch.arange(9))


# ------------------------------------------------------------------------------------------------- the selection helper
def test_selection_helper():
    from ttx_dense import dense_table_flags, dense_table_groups

    Es = [3, 200000, 1460, 24, 50000, 583]
    assert dense_table_flags(Es) == [False] * 6 and dense_table_groups(dense_table_flags(Es)) == []
    assert dense_table_flags(Es, dense_below=10000) == [True, False, True, True, False, True]
    assert dense_table_flags(Es, dense_below=1460) == [True, False, False, True, False, True], "strictly below"
    assert dense_table_flags(Es, 10000, dense=[False, True, False, False, False, False]) == [False, True] + [False] * 4, \
        "`dense` overrides dense_below"
    assert dense_table_groups([True, False, True, True, False, True]) == [[0, 2, 3, 5]]
    with pytest.raises(ValueError):
        dense_table_flags(Es, dense=[True])
    with pytest.raises(ValueError):
        dense_table_flags(Es, dense_below=-1)
    many = dense_table_groups([True] * 70 + [False] + [True] * 60)
    assert [len(g) for g in many] == [64, 64, 2] and many[1][:7] == [64, 65, 66, 67, 68, 69, 71] and many[2] == [129, 130]
    criteo = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10, 5652, 2173,
              4, 7046547, 18, 15, 286181, 105, 142572]
    assert sum(dense_table_flags(criteo, 10000)) == 16 and sum(dense_table_flags(criteo, 10 ** 6)) == 21


def test_mixed_module_accepts_the_keywords():
    import inspect

    import ttx_mixed

    sig = inspect.signature(ttx_mixed.MixedTTEmbeddingBag.__init__)
    assert sig.parameters["dense_below"].default == 0 and sig.parameters["dense"].default is None


# --------------------------------------------------------------------------------------------------- the compiler report
def test_dense_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed); the figures are in DESIGN.md 4.16"""
    from test_kernel_resources import resources

    res = resources("ttx_dense.hip")
    names = sorted(k for k in res if "dense_" in k)
    for w in ("dense_fwd_kernelILi4ELi0", "dense_fwd_kernelILi4ELi1", "dense_fwd_kernelILi4ELi2", "dense_fwd_kernelILi1ELi0",
              "dense_fwd_kernelILi1ELi1", "dense_fwd_kernelILi1ELi2", "dense_keys_kernel", "dense_psw_grad_kernelILi4",
              "dense_psw_grad_kernelILi1", "dense_partial_kernelILi4", "dense_partial_kernelILi1", "dense_apply_kernelILi4",
              "dense_apply_kernelILi1"):
        assert sum(w in k for k in names) == 1, (w, names)
    assert len(names) == 13, names
    for k in names:
        print(k, res[k])
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        assert res[k]["VGPRs"] <= 128 and res[k]["Occupancy"] >= 4, (k, res[k])
