"""The MFMA-tail bf16 inference forward without a GPU: the shapes it takes (the default factorings of every
width from 640 up), every argument error of its entry points before a device is touched, and
TTInferenceBag.from_module(m, mfma_tail=True) on CPU tensors (the torch-op path) within the derived bound of tests/bf16_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G
from test_bf16_infer_cpu import P_SMALL, _bags, _libs, _module, ops  # noqa: F401  (ops: the oracle-engine fixture)

DEFAULT_Q = [[8, 8, 10], [8, 8, 12], [8, 8, 16], [8, 10, 16], [8, 12, 16], [8, 16, 16], [16, 16, 16], [16, 16, 32]]
SHAPES = [([2, 2, 16], [16, 16]), ([8, 8, 16], [32, 32]), ([3, 5, 10], [40, 33]), ([4, 4, 32], [64, 64]), ([16, 16, 16], [64, 128])]
i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t


def _mfma_libs():
    import tt_embeddings as E

    G_ = ctypes.POINTER(E._Geom)
    for lib in _libs():
        lib.ttx_tt_rows_bf16m_supported.argtypes = [G_]
        lib.ttx_tt_pack_bf16m_elems.restype = i64
        lib.ttx_tt_pack_bf16m_elems.argtypes = [G_, i32]
        lib.ttx_tt_pack_bf16m.argtypes = [G_, i32, vp, vp, vp]
        lib.ttx_tt_rows_bf16m_workspace_bytes.restype = sz
        lib.ttx_tt_rows_bf16m_workspace_bytes.argtypes = [G_, i32, i64]
        lib.ttx_tt_rows_bf16m.argtypes = [G_, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]
        yield lib


def test_supported_shapes():
    import tt_embeddings as E

    shapes = SHAPES + [(q, [rk, rk]) for q in DEFAULT_Q for rk in (16, 32, 64)] + [([8, 8, 16], [128, 128]), ([16, 16, 16], [128, 128])]
    for q, r in shapes:
        for tables, p in ((1, [5, 6, 7]), (3, [7, 9, 11]), (0, [[5, 6, 7], [7, 9, 11], [2, 3, 4]])):
            assert E.tt_rows_bf16m_supported(tables, p, q, [1] + r + [1]), (q, r)
    for T in (2, 4):
        p, q, r = G.test_shape(T)
        assert not E.tt_rows_bf16m_supported(1, p, q, [1] + list(r) + [1])
    assert not E.tt_rows_bf16m_supported(1, P_SMALL, [4, 4, 16], [1, 129, 128, 1])
    assert not E.tt_rows_bf16m_supported(1, P_SMALL, [4, 4, 16], [1, 128, 129, 1])
    assert not E.tt_rows_bf16m_supported(1, P_SMALL, [4, 4, 33], [1, 32, 32, 1])
    assert not E.tt_rows_bf16m_supported(1, P_SMALL, [16, 64, 16], [1, 32, 128, 1])  # x_0 of a lookup: 1024 rows of 272 B
    assert E.tt_rows_bf16m_supported(1, P_SMALL, [16, 64, 16], [1, 32, 32, 1])       # (1024 rows of 80 B fit)
    for lib in _mfma_libs():
        assert lib.ttx_tt_rows_bf16m_supported(None) == 0
        g = E._geom(1, P_SMALL, [3, 5, 10], [1, 40, 33, 1])  # K1p = 64, N1p = 176, Q2P = 16, K2p = 64
        assert [lib.ttx_tt_pack_bf16m_elems(ctypes.byref(g), t) for t in (0, 1, 2, 3, -1)] == [5 * 3 * 64, 6 * 176 * 64, 7 * 16 * 64, 0, 0]


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced: a call that reached the runtime without a GPU would return -4)"""
    import tt_embeddings as E

    fake, odd = 4096, 4100
    g = E._geom(2, P_SMALL, [8, 8, 16], [1, 32, 32, 1])
    refused = [(E._geom(1, *[list(x) for x in G.test_shape(T)[:2]], [1] + list(G.test_shape(T)[2]) + [1]), int(np.prod(G.test_shape(T)[1])))
               for T in (2, 4)] + [(E._geom(1, P_SMALL, [4, 4, 16], [1, 129, 128, 1]), 256), (E._geom(1, P_SMALL, [4, 4, 33], [1, 32, 32, 1]), 528),
                                   (E._geom(1, P_SMALL, [16, 64, 16], [1, 32, 128, 1]), 16384)]
    for lib in _mfma_libs():
        need = lib.ttx_tt_rows_bf16m_workspace_bytes(ctypes.byref(g), 1024, 100)
        assert need > 0 and lib.ttx_tt_rows_bf16m_workspace_bytes(ctypes.byref(refused[0][0]), refused[0][1], 100) == 0

        def rows(**kw):
            a = dict(g=ctypes.byref(g), D=1024, nnz=100, idx=fake, tab=fake, pc=(vp * 3)(fake, fake, fake), rows=fake, plan=None,
                     ws=fake, wsb=need)
            a.update(kw)
            return lib.ttx_tt_rows_bf16m(a["g"], a["D"], a["nnz"], a["idx"], a["tab"], a["pc"], a["rows"], a["plan"], a["ws"],
                                         a["wsb"], None)

        for kw in [dict(g=None), dict(D=1023), dict(D=0), dict(nnz=-1), dict(nnz=1 << 31), dict(pc=None), dict(pc=(vp * 3)(fake, None, fake)),
                   dict(pc=(vp * 3)(None, fake, fake)), dict(pc=(vp * 3)(fake, fake, 0)), dict(pc=(vp * 3)(odd, fake, fake)),
                   dict(rows=None), dict(rows=odd), dict(rows=fake + 8), dict(idx=None)]:
            assert rows(**kw) == -1 and lib.ttx_last_error(), kw
        for kw in (dict(wsb=need - 257), dict(wsb=0), dict(ws=None)):
            assert rows(**kw) == -2, kw  # TTX_EWORKSPACE
        for gg, D in refused:
            assert rows(g=ctypes.byref(gg), D=D) == -3  # TTX_EUNSUPPORTED
            assert lib.ttx_tt_pack_bf16m(ctypes.byref(gg), 0, fake, fake, None) == -3
        assert rows(nnz=0, idx=None, pc=None, rows=None, ws=None, wsb=0) == 0
        for kw in (dict(t=3), dict(t=-1), dict(src=None), dict(dst=None), dict(dst=fake + 8), dict(src=fake + 2), dict(g=None)):
            a = dict(g=ctypes.byref(g), t=1, src=fake, dst=fake)
            a.update(kw)
            assert lib.ttx_tt_pack_bf16m(a["g"], a["t"], a["src"], a["dst"], None) == -1, kw


@pytest.mark.parametrize("q,r", [SHAPES[1], SHAPES[2]])
def test_from_module_mfma_tail_on_cpu_tensors(ops, q, r):
    import ttx_infer

    for kind, tables, mode in (("batched", 3, "mean"), ("bag", 1, "sum")):
        m, E, D = _module(ops, kind, tables, q, r, mode=mode)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        assert ttx_infer.TTInferenceBag.from_module(m).route == "fp32"
        inf = ttx_infer.TTInferenceBag.from_module(m, mfma_tail=True)
        assert inf.route == "bf16m" and not list(inf.parameters()) and all(b.dtype == torch.bfloat16 for b in inf.buffers())
        assert inf.packed_core2.numel() == tables * P_SMALL[2] * 16 * (-(-r[1] // 32) * 32)  # [Q2P][K2p]
        cores = [R.to_bf16(c.detach().numpy()) for c in m.tt_cores]
        idx, off = _bags(np.random.RandomState(7), tables, 6, E)
        out = inf(torch.from_numpy(idx), torch.from_numpy(off))
        tab = np.repeat(np.arange(tables * 6) // 6, np.diff(off))
        ref, bnd = R.pool64(*R.rows64(*R.slices(cores, P_SMALL, q, r, idx, tab)), off, mean=mode == "mean")
        err = np.abs(out.numpy().astype(np.float64).reshape(ref.shape) - ref)
        assert (err <= bnd).all(), f"{kind} {mode}: worst err / bound {np.max(err / np.maximum(bnd, 1e-300)):.3f}"
        after = m.state_dict()
        assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    # a geometry the other kernels take keeps its route with the flag
    narrow = _module(ops, "bag", 1, [2, 2, 4], [16, 16])[0]
    assert ttx_infer.TTInferenceBag.from_module(narrow, mfma_tail=True).route == "bf16"
    wide = _module(ops, "bag", 1, [4, 4, 4], [128, 128])[0]
    assert ttx_infer.TTInferenceBag.from_module(wide, wide=True, mfma_tail=True).route == "bf16w"
