"""The bf16 inference forward without a GPU: TTInferenceBag's torch-op path against the float64 chain product on
the bf16 cores within the derived bound (tests/bf16_ref.py); the fp32 fall-back on the oracle engine; every refusal of
from_module; the packed layout with torch ops; the ABI (declared, exported, argument errors before a device is touched, the
supported shapes); and the compiler's resource report of the new kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G
import oracle_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = [("int", "ttx_tt_rows_bf16_supported"), ("int64_t", "ttx_tt_pack_bf16_elems"), ("int", "ttx_tt_pack_bf16"),
                ("size_t", "ttx_tt_rows_bf16_workspace_bytes"), ("int", "ttx_tt_rows_bf16"), ("int", "ttx_bag_sum_pool")]
P_SMALL = [5, 6, 7]


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


def _module(ops, kind, tables, q, r, p=P_SMALL, dist="signed", seed=3, **kw):
    E, D = int(np.prod(p)), int(np.prod(q))
    if kind == "batched":
        m = ops.TableBatchedTTEmbeddingBag(tables, E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu", **kw)
    elif kind == "bag":
        m = ops.TTEmbeddingBag(E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu",
                               **{"use_cache": False, **kw})
    else:
        m = ops.TTEmbedding(E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu", **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, G.make_cores(seed, m.num_tables, p, q, r, dist)):
            dst.copy_(torch.from_numpy(src))
    return m, E, D


def _bags(rs, tables, B, E):
    lens = rs.randint(0, 5, size=tables * B)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rs.randint(0, E, size=int(off[-1])).astype(np.int64), off


# ------------------------------------------------------------------------------------------------------ the torch-op path
@pytest.mark.parametrize("q,r", R.SHAPES)
@pytest.mark.parametrize("dist", ["uniform", "signed"])
def test_torch_path_meets_the_bound(ops, q, r, dist):
    import ttx_infer

    worst = 0.0
    for kind, tables, mode in (("batched", 3, "sum"), ("batched", 1, "mean"), ("bag", 1, "sum"), ("embedding", 1, "sum")):
        kw = {} if kind == "embedding" else dict(mode=mode)
        m, E, D = _module(ops, kind, tables, q, r, dist=dist, **kw)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        inf = ttx_infer.TTInferenceBag.from_module(m)
        assert inf.route == "bf16" and not list(inf.parameters())
        assert all(b.dtype == torch.bfloat16 for b in inf.buffers())
        cores = [R.to_bf16(c.detach().numpy()) for c in m.tt_cores]
        rs = np.random.RandomState(7)
        if kind == "embedding":
            idx = rs.randint(0, E, size=(3, 5)).astype(np.int64)
            out = inf(torch.from_numpy(idx))
            assert tuple(out.shape) == (3, 5, D)
            ref, bnd = R.rows64(*R.slices(cores, P_SMALL, q, r, idx.reshape(-1), np.zeros(idx.size, np.int64)))
        else:
            B = 6
            idx, off = _bags(rs, tables, B, E)
            out = inf(torch.from_numpy(idx), torch.from_numpy(off))
            assert tuple(out.shape) == ((B, D) if kind == "bag" else (tables, B, D))
            tab = np.repeat(np.arange(tables * B) // B, np.diff(off))
            rows, rb = R.rows64(*R.slices(cores, P_SMALL, q, r, idx, tab))
            ref, bnd = R.pool64(rows, rb, off, mean=mode == "mean")
        assert out.dtype == torch.float32 and not out.requires_grad
        err = np.abs(out.numpy().astype(np.float64).reshape(ref.shape) - ref)
        assert (err <= bnd).all(), f"{kind} {mode}: worst err / bound {np.max(err / np.maximum(bnd, 1e-300)):.3f}"
        worst = max(worst, float(np.max(err / np.maximum(bnd, 1e-300))))
        after = m.state_dict()
        assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    print(f"q={q} r={r} {dist}: worst err / bound on the torch path {worst:.4f}")


def test_bound_catches_a_dropped_term():
    """the bound is tight enough to see one missing k2 term on most elements (the contract's own check of itself)"""
    q, r = [4, 4, 4], [32, 32]
    for dist in ("uniform", "signed"):
        cores = [R.to_bf16(c) for c in G.make_cores(5, 1, P_SMALL, q, r, dist)]
        idx = np.random.RandomState(1).randint(0, int(np.prod(P_SMALL)), size=40)
        A, B, C = R.slices(cores, P_SMALL, q, r, idx, np.zeros(40, np.int64))
        ref, bnd = R.rows64(A, B, C)
        C2 = C.copy()
        C2[:, 5, :] = 0.0  # drop k2 = 5
        wrong, _ = R.rows64(A, B, C2)
        assert (np.abs(wrong - ref) > bnd).mean() > 0.5


@pytest.mark.parametrize("T,r", [(2, None), (4, None), (3, [128, 128])])
def test_fp32_fallback_serves_the_rounded_weights(ops, T, r):
    import ttx_infer

    if r is None:
        p, q, r = G.test_shape(T)
    else:
        p, q = P_SMALL, [2, 2, 2]
    E, D = int(np.prod(p)), int(np.prod(q))
    m = ops.TableBatchedTTEmbeddingBag(2, E, D, list(r), list(p), list(q), weight_dist="uniform", device="cpu")
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    inf = ttx_infer.TTInferenceBag.from_module(m)
    assert inf.route == "fp32" and not list(inf.parameters())
    assert all(torch.equal(sd0[k], v) for k, v in m.state_dict().items())
    idx, off = _bags(np.random.RandomState(2), 2, 5, E)
    out = inf(torch.from_numpy(idx), torch.from_numpy(off))
    assert not out.requires_grad and tuple(out.shape) == (2, 5, D)
    with torch.no_grad():
        for c in m.tt_cores:
            c.copy_(c.to(torch.bfloat16).float())
        ref = m(torch.from_numpy(idx), torch.from_numpy(off))
    assert torch.equal(out, ref)


def test_every_refusal_of_from_module(ops):
    import ttx_infer
    import ttx_mixed

    F = ttx_infer.TTInferenceBag.from_module
    q, r = [2, 2, 4], [16, 16]
    with pytest.raises(ValueError, match="max"):
        F(_module(ops, "batched", 2, q, r, mode="max")[0])
    with pytest.raises(ValueError, match="padding_idx"):
        F(_module(ops, "batched", 1, q, r, padding_idx=3)[0])
    with pytest.raises(ValueError, match="padding_idx"):
        F(_module(ops, "embedding", 1, q, r, padding_idx=0)[0])
    m, E, D = _module(ops, "bag", 1, q, r, use_cache=True, cache_size=8, hashtbl_size=64)
    F(m)  # (a cache that is still warming up holds no trained rows)
    m.warmup = False
    with pytest.raises(ValueError, match=r"cache_populate\(write_back"):
        F(m)
    with pytest.raises(TypeError):
        F(torch.nn.EmbeddingBag(10, 8))
    with pytest.raises(TypeError):
        F(ttx_mixed.VarTableTTEmbeddingBag([100, 90], 16, r, [[4, 5, 5], [4, 5, 5]], q, weight_dist="uniform", device="cpu"))
    inf = F(_module(ops, "batched", 2, q, r)[0])
    with pytest.raises(ValueError):
        inf(torch.zeros(4, dtype=torch.float32), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        inf(torch.zeros(4, dtype=torch.int64), torch.tensor([0, 2, 4, 4]))  # 3 bags for 2 tables
    # call forms: int32, bag starts only, [N, L]
    m, E, D = _module(ops, "batched", 2, q, r, include_last_offset=False)
    inf = F(m)
    idx = torch.arange(12, dtype=torch.int64) % E
    a = inf(idx, torch.tensor([0, 3, 6, 9]))
    assert torch.equal(a, inf(idx.int(), torch.tensor([0, 3, 6, 9], dtype=torch.int32))) and torch.equal(a, inf(idx.view(4, 3)))
    assert tuple(inf(idx[:0], torch.zeros(4, dtype=torch.int64)).shape) == (2, 2, D)


def test_packed_layout_with_torch_ops():
    """pack_cores_torch writes the layout ttx.h documents, and unpack gives the bf16 values back"""
    import ttx_infer

    q, r = [3, 4, 5], [13, 12]
    cores = [torch.from_numpy(c) for c in G.make_cores(9, 2, P_SMALL, q, r, "signed")]
    pk = ttx_infer.pack_cores_torch(cores, q, [1] + r + [1])
    K1p, N1p = 32, 48
    assert [x.numel() for x in pk] == [2 * 5 * 3 * K1p, 2 * 6 * N1p * K1p, 2 * 7 * 12 * 8]
    c1 = cores[1].view(12, 13, 4, 12).to(torch.bfloat16)
    p1 = pk[1].view(12, N1p, K1p)
    assert p1[7, 2 * 12 + 5, 9] == c1[7, 9, 2, 5] and not p1[:, :, 13:].any()
    assert pk[0].view(10, 3, K1p)[4, 2, 11] == cores[0].view(10, 3, 13).to(torch.bfloat16)[4, 2, 11]
    assert pk[2].view(14, 12, 8)[3, 7, 4] == cores[2].view(14, 12, 5).to(torch.bfloat16)[3, 7, 4] and not pk[2].view(14, 12, 8)[:, :, 5:].any()
    back = ttx_infer.unpack_cores_torch(pk, q, [1] + r + [1])
    for b, c in zip(back, cores):
        assert torch.equal(b, c.view(-1, c.size(-1)).to(torch.bfloat16).float())


# --------------------------------------------------------------------------------------------------------------- the ABI
i32, i64, vp, sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t


def _libs():
    import tt_embeddings as E

    G_ = ctypes.POINTER(E._Geom)
    for name in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", name))
        lib.ttx_last_error.restype = ctypes.c_char_p
        lib.ttx_tt_rows_bf16_supported.argtypes = [G_]
        lib.ttx_tt_pack_bf16_elems.restype = i64
        lib.ttx_tt_pack_bf16_elems.argtypes = [G_, i32]
        lib.ttx_tt_pack_bf16.argtypes = [G_, i32, vp, vp, vp]
        lib.ttx_tt_rows_bf16_workspace_bytes.restype = sz
        lib.ttx_tt_rows_bf16_workspace_bytes.argtypes = [G_, i32, i64]
        lib.ttx_tt_rows_bf16.argtypes = [G_, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]
        lib.ttx_bag_sum_pool.argtypes = [i64, i32, vp, vp, vp, vp]
        yield lib


def test_entry_points_are_declared_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    for ret, name in ENTRY_POINTS:
        assert re.search(r"\b%s\s+%s\s*\(" % (ret, name), hdr), name
    for lib in _libs():
        for _, name in ENTRY_POINTS:
            assert getattr(lib, name) is not None
    import tt_embeddings as E

    for name in ("pack_cores_bf16", "tt_rows_bf16", "tt_rows_bf16_supported", "bag_sum_pool"):
        assert callable(getattr(E, name))
    with pytest.raises(RuntimeError):  # (no CPU path in the engine)
        E.bag_sum_pool(torch.zeros(2, 4), torch.tensor([0, 2]))


def test_supported_shapes():
    import tt_embeddings as E

    for q, r in R.SHAPES:
        for tables, p in ((1, [5, 6, 7]), (3, [7, 9, 11]), (26, [200, 220, 250]), (1, [1, 1, 1])):
            assert E.tt_rows_bf16_supported(tables, p, q, [1] + r + [1])
        assert E.tt_rows_bf16_supported(0, [[5, 6, 7], [7, 9, 11], [2, 3, 4]], q, [1] + r + [1])  # p_tables
    p2, q2, r2 = G.test_shape(2)
    p4, q4, r4 = G.test_shape(4)
    assert not E.tt_rows_bf16_supported(1, p2, q2, [1] + list(r2) + [1])
    assert not E.tt_rows_bf16_supported(1, p4, q4, [1] + list(r4) + [1])
    assert not E.tt_rows_bf16_supported(1, P_SMALL, [4, 4, 4], [1, 128, 128, 1])
    assert not E.tt_rows_bf16_supported(1, P_SMALL, [4, 4, 4], [1, 65, 32, 1])
    assert not E.tt_rows_bf16_supported(1, P_SMALL, [4, 4, 9], [1, 32, 32, 1])      # q2 beyond the tail's registers
    assert not E.tt_rows_bf16_supported(1, P_SMALL, [4, 64, 4], [1, 32, 64, 1])     # the x_0 tile does not fit the LDS
    for lib in _libs():
        assert lib.ttx_tt_rows_bf16_supported(None) == 0
        g = E._geom(1, P_SMALL, [4, 4, 8], [1, 64, 64, 1])
        assert [lib.ttx_tt_pack_bf16_elems(ctypes.byref(g), t) for t in (0, 1, 2, 3, -1)] == \
            [5 * 4 * 64, 6 * 256 * 64, 7 * 64 * 8, 0, 0]


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced; this machine has no GPU: a call that reached the runtime would return -4)"""
    import tt_embeddings as E

    fake, odd = 4096, 4100
    g = E._geom(2, P_SMALL, [4, 4, 4], [1, 32, 32, 1])
    g2 = E._geom(1, *[list(x) for x in G.test_shape(2)[:2]], [1] + list(G.test_shape(2)[2]) + [1])
    g4 = E._geom(1, *[list(x) for x in G.test_shape(4)[:2]], [1] + list(G.test_shape(4)[2]) + [1])
    gbig = E._geom(1, P_SMALL, [4, 4, 4], [1, 128, 128, 1])
    for lib in _libs():
        need = lib.ttx_tt_rows_bf16_workspace_bytes(ctypes.byref(g), 64, 100)
        assert need > 0 and lib.ttx_tt_rows_bf16_workspace_bytes(ctypes.byref(g2), 12, 100) == 0

        def rows(**kw):
            a = dict(g=ctypes.byref(g), D=64, nnz=100, idx=fake, tab=fake, pc=(vp * 3)(fake, fake, fake), rows=fake, plan=None,
                     ws=fake, wsb=need)
            a.update(kw)
            return lib.ttx_tt_rows_bf16(a["g"], a["D"], a["nnz"], a["idx"], a["tab"], a["pc"], a["rows"], a["plan"], a["ws"],
                                        a["wsb"], None)

        bad = [dict(g=None), dict(D=63), dict(D=0), dict(nnz=-1), dict(nnz=1 << 31), dict(pc=None), dict(pc=(vp * 3)(fake, None, fake)),
               dict(pc=(vp * 3)(None, fake, fake)), dict(pc=(vp * 3)(fake, fake, 0)), dict(pc=(vp * 3)(odd, fake, fake)),
               dict(rows=None), dict(rows=odd), dict(rows=fake + 8), dict(idx=None)]
        for kw in bad:
            assert rows(**kw) == -1, kw
            assert lib.ttx_last_error(), kw
        for kw in (dict(wsb=need - 257), dict(wsb=0), dict(ws=None)):
            assert rows(**kw) == -2, kw  # TTX_EWORKSPACE
        for gg, D in ((g2, 12), (g4, 420), (gbig, 64)):
            assert rows(g=ctypes.byref(gg), D=D) == -3  # TTX_EUNSUPPORTED
            assert lib.ttx_tt_pack_bf16(ctypes.byref(gg), 0, fake, fake, None) == -3
        assert rows(nnz=0, idx=None, pc=None, rows=None, ws=None, wsb=0) == 0

        for kw in (dict(t=3), dict(t=-1), dict(src=None), dict(dst=None), dict(dst=fake + 8), dict(src=fake + 2), dict(g=None)):
            a = dict(g=ctypes.byref(g), t=1, src=fake, dst=fake)
            a.update(kw)
            assert lib.ttx_tt_pack_bf16(a["g"], a["t"], a["src"], a["dst"], None) == -1, kw

        def pool(**kw):
            a = dict(nb=4, D=8, off=fake, rows=fake, out=fake)
            a.update(kw)
            return lib.ttx_bag_sum_pool(a["nb"], a["D"], a["off"], a["rows"], a["out"], None)

        for kw in (dict(nb=-1), dict(nb=1 << 31), dict(D=0), dict(D=-4), dict(off=None), dict(rows=None), dict(out=None),
                   dict(off=odd), dict(rows=fake + 2), dict(out=fake + 1)):
            assert pool(**kw) == -1, kw
            assert b"bag_sum_pool" in lib.ttx_last_error()
        assert pool(nb=0, off=None, rows=None, out=None) == 0


# --------------------------------------------------------------------------------------------------- the compiler report
def test_bf16_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed); the figures are in DESIGN.md 4.19"""
    from test_kernel_resources import resources

    res = resources("ttx_tt_bf16.hip")
    names = sorted(res)
    rows = [f"tt_rows_bf16_kernelILi{kb}ELi{q2p}ELb{st}E" for kb in (1, 2) for q2p in (4, 8) for st in (0, 1)]
    for w in ["pack_bf16_kernel", "bag_sum_pool_kernelIf", "bag_sum_pool_kernelI15HIP_vector_type"] + rows:
        assert sum(w in k for k in names) == 1, (w, names)
    assert len(names) == 11, names
    for k in names:
        print(k, res[k])
        assert res[k]["ScratchSize"] == 0, (k, res[k])
        if "tt_rows_bf16" in k:
            assert res[k]["VGPRs"] <= 128 and res[k]["Occupancy"] >= 3, (k, res[k])  # (three work-groups of 4 waves per CU at least)
