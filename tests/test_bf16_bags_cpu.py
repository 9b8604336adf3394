"""The pooled one-launch bf16 forward without a GPU: the shapes it takes and refuses, the ABI, the route of
TTInferenceBag.from_module(m, fused_bags=True) on CPU tensors within the bound of tests/bf16b_ref.py, the unit's resource report."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bf16_ref as R
import bf16b_ref as RB
import gen_inputs as G
from test_bf16_infer_cpu import P_SMALL, ROOT, _bags, _libs, _module, ops  # noqa: F401  (ops: the oracle-engine fixture)
from test_bf16_infer_gpu import _pad

SHAPES = [([4, 4, 4], [32, 32]), ([3, 4, 5], [13, 12]), ([4, 4, 8], [64, 64]), ([2, 4, 32], [16, 16]), ([8, 8, 4], [32, 32])]
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


def test_supported_shapes_and_refusals():
    import tt_embeddings as E

    for q, r in SHAPES:
        for tables, p in ((1, [5, 6, 7]), (3, [7, 9, 11]), (26, [200, 220, 250])):
            assert E.tt_bags_bf16_supported(tables, p, q, _pad(r)), (q, r)
        assert not E.tt_bags_bf16_supported(0, [[5, 6, 7], [7, 9, 11], [2, 3, 4]], q, _pad(r))  # p_tables
    small = (([4, 4, 4], [128, 32]), ([4, 4, 4], [32, 128]), ([8, 16, 4], [32, 32]), ([4, 4, 64], [32, 32]), ([32, 2, 4], [16, 16]))
    for p, q, r in [G.test_shape(2), G.test_shape(4)] + [(P_SMALL, q, r) for q, r in small]:
        assert not E.tt_bags_bf16_supported(1, list(p), list(q), _pad(r)), (q, r)


def test_abi_and_argument_errors_before_a_device_is_touched():
    """(the pointers below are never dereferenced: a call that reached the runtime without a GPU would return -4)"""
    import tt_embeddings as E

    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    assert all(re.search(r"\bint\s+%s\s*\(" % n, hdr) for n in ("ttx_tt_bags_bf16_supported", "ttx_tt_bags_bf16")) and callable(E.tt_bags_bf16)
    fake, odd = 4096, 4100
    g = E._geom(2, P_SMALL, [4, 4, 4], [1, 32, 32, 1])
    refused = [(E._geom(1, *[list(x) for x in G.test_shape(T)[:2]], _pad(G.test_shape(T)[2])), int(np.prod(G.test_shape(T)[1]))) for T in (2, 4)]
    refused += [(E._geom(1, P_SMALL, [4, 4, 4], [1, 128, 128, 1]), 64), (E._geom(1, P_SMALL, [8, 16, 4], [1, 32, 32, 1]), 512),
                (E._geom(0, [[5, 6, 7], [7, 9, 11]], [4, 4, 4], [1, 32, 32, 1]), 64)]
    for lib in _libs():
        G_ = ctypes.POINTER(E._Geom)
        lib.ttx_tt_bags_bf16_supported.argtypes = [G_]
        lib.ttx_tt_bags_bf16.argtypes = [G_, i32, i64, i64, vp, vp, vp, i64, i32, vp, vp, vp]
        assert lib.ttx_tt_bags_bf16_supported(None) == 0 and lib.ttx_tt_bags_bf16_supported(ctypes.byref(g)) == 1

        def bags(**kw):
            a = dict(g=ctypes.byref(g), D=64, nb=8, nnz=100, idx=fake, off=fake, w=None, pad=-1, mean=0, pc=(vp * 3)(fake, fake, fake), out=fake)
            a.update(kw)
            return lib.ttx_tt_bags_bf16(a["g"], a["D"], a["nb"], a["nnz"], a["idx"], a["off"], a["w"], a["pad"], a["mean"], a["pc"],
                                        a["out"], None)

        for kw in [dict(g=None), dict(D=63), dict(D=0), dict(nb=-2), dict(nb=7), dict(nb=1 << 31), dict(nnz=-1), dict(nnz=1 << 31),
                   dict(w=fake, mean=1), dict(pad=-2), dict(idx=None), dict(off=None), dict(out=None), dict(pc=None),
                   dict(pc=(vp * 3)(fake, None, fake)), dict(pc=(vp * 3)(odd, fake, fake)), dict(idx=odd), dict(off=odd), dict(w=fake + 2),
                   dict(out=fake + 2)]:
            assert bags(**kw) == -1 and b"tt_bags_bf16" in lib.ttx_last_error(), kw
        for gg, D in refused:
            assert bags(g=ctypes.byref(gg), D=D) == -3 and b"q0 q1 <= 64" in lib.ttx_last_error()  # TTX_EUNSUPPORTED names the domain
        assert bags(nb=0, nnz=0, idx=None, off=None, out=None, pc=None) == 0


@pytest.mark.parametrize("q,r", [SHAPES[1], SHAPES[3]])
def test_from_module_fused_bags_on_cpu_tensors(ops, q, r):
    import ttx_infer

    F = ttx_infer.TTInferenceBag.from_module
    rs = np.random.RandomState(7)
    for kind, tables, mode, pad in (("batched", 3, "mean", 2), ("bag", 1, "sum", None), ("batched", 2, "sum", 0)):
        m, E, D = _module(ops, kind, tables, q, r, mode=mode, **({} if pad is None else dict(padding_idx=pad)))
        with pytest.raises(ValueError, match="padding_idx" if pad is not None else "fused_bags=True"):  # (without the flag)
            F(m)(torch.zeros(4, dtype=torch.int64), torch.tensor([0, 4]), torch.ones(4))
        inf = F(m, fused_bags=True)
        assert inf.route == "bf16b" and inf.padding_idx == pad and list(inf.state_dict()) == ["packed_core0", "packed_core1", "packed_core2"]
        assert inf.packed_core2.numel() == tables * P_SMALL[2] * (-(-q[2] // 16) * 16) * 32  # the MFMA-tail layout [Q2P][K2p]
        cores = [R.to_bf16(c.detach().numpy()) for c in m.tt_cores]
        idx, off = _bags(rs, tables, 5, E)
        idx[rs.rand(idx.size) < 0.3] = E - 1 if pad is None else pad
        w = rs.uniform(-2, 2, size=idx.size).astype(np.float32)
        for ww in ([None, w] if mode == "sum" else [None]):
            out = inf(torch.from_numpy(idx), torch.from_numpy(off), None if ww is None else torch.from_numpy(ww))
            ref, bnd = RB.bags64(cores, P_SMALL, q, r, tables, idx, off, ww, pad, mode == "mean")
            err = np.abs(out.numpy().astype(np.float64).reshape(ref.shape) - ref)
            assert (err <= bnd).all(), f"{kind} {mode}: worst err / bound {np.max(err / np.maximum(bnd, 1e-300)):.3f}"
        bad = [(w, "mode='sum'")] if mode == "mean" else [(w[:-1], "shape of indices"), (w.astype(np.float64), "float32")]
        for ww, what in bad:
            with pytest.raises(ValueError, match=what):
                inf(torch.from_numpy(idx), torch.from_numpy(off), torch.from_numpy(ww))
    assert F(_module(ops, "embedding", 1, q, r)[0], fused_bags=True).route == F(_module(ops, "embedding", 1, q, r)[0]).route
    assert F(_module(ops, "bag", 1, [4, 4, 4], [128, 128])[0], fused_bags=True).route == "fp32"
    with pytest.raises(ValueError, match="max"):
        F(_module(ops, "batched", 2, q, r, mode="max")[0], fused_bags=True)
    with pytest.raises(ValueError, match="hot row table.*fused_bags"):
        F(_module(ops, "bag", 1, q, r)[0], fused_bags=True, hot_indices=torch.arange(4))


def test_every_instantiation_compiles_without_scratch():
    from test_kernel_resources import resources

    res = resources("ttx_tt_bags_bf16.hip")  # (the compiler's own report for gfx950; the figures are in DESIGN.md 4.25)
    names = [f"tt_bags_bf16_kernelILi{kb}ELi{k2b}ELi{mq}E" for kb in (1, 2) for k2b in (1, 2) for mq in (1, 2)]
    assert len(res) == len(names) and all(sum(w in k for k in res) == 1 for w in names), sorted(res)
    for k, v in sorted(res.items()):
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
