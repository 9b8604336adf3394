"""dense_rows and the expand kernel's entry points without a GPU: CPU modules against ttx_svd.tt_full, the
domain of tt_expand_supported at its edges, every argument error before a device is touched, and the compiler's resource report."""
import ctypes

import pytest
import torch

import gen_inputs as G
from test_bf16_infer_cpu import _libs, _module, ops  # noqa: F401  (ops: the oracle-engine fixture)

P = [3, 4, 37]
i32, i64, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p


@pytest.mark.parametrize("kind,tables", [("batched", 3), ("bag", 1), ("embedding", 1)])
def test_dense_rows_on_cpu_modules_equals_tt_full(ops, kind, tables):
    import ttx_svd

    m, E, D = _module(ops, kind, tables, [3, 4, 5], [13, 12], p=P)
    for k in range(tables):
        full = ttx_svd.tt_full(m.table_cores(k), E)
        for start, stop in ((0, None), (5, 6), (40, 70), (7, 7)):
            got = m.dense_rows(start, stop, table=k)
            assert not got.requires_grad and torch.equal(got, full[start:stop])
    out = torch.full((30, D), float("nan"))
    assert m.dense_rows(40, 70, out=out) is out and torch.equal(out, ttx_svd.tt_full(m.table_cores(0), E)[40:70])
    for bad in (dict(stop=E + 1), dict(start=-1), dict(start=9, stop=8), dict(table=tables)):
        with pytest.raises(IndexError):
            m.dense_rows(**bad)
    for bad in (torch.empty(30, D, dtype=torch.float64), torch.empty(29, D), torch.empty(D, 30).t()):
        with pytest.raises(ValueError):
            m.dense_rows(40, 70, out=bad)
    m.use_cache, m.warmup = True, False  # (what a populated cache leaves behind)
    with pytest.raises(ValueError, match="row cache is live"):
        m.dense_rows()


def test_supported_domain_at_its_edges():
    import tt_embeddings as E

    for tables, p in ((1, P), (3, P), (0, [P, [7, 9, 11]])):
        for q, r in (([4, 4, 4], [32, 32]), ([3, 4, 5], [13, 12]), ([16, 51, 32], [128, 12]), ([16, 4, 32], [1, 128]), ([8, 8, 16], [128, 128])):
            assert E.tt_expand_supported(tables, p, q, [1] + r + [1]), (q, r)
    for q, r in (([4, 4, 4], [129, 32]), ([4, 4, 4], [32, 129]), ([17, 4, 4], [8, 8]), ([4, 65, 4], [8, 8]), ([4, 4, 33], [8, 8]),
                 ([16, 52, 4], [8, 16]),      # x_0 of a prefix: 832 rows of 20 floats = 65 KiB (816 rows fit: above)
                 ([16, 8, 16], [128, 128])):  # 128 rows of 132 floats = 66 KiB
        assert not E.tt_expand_supported(1, P, q, [1] + r + [1]), (q, r)
    for T in (2, 4):
        p, q, r = G.test_shape(T)
        assert not E.tt_expand_supported(1, p, q, [1] + list(r) + [1])


def test_every_argument_error_returns_minus_one_before_a_device_is_touched():
    """(the pointers below are never dereferenced: a call that reached the runtime without a GPU would return -4)"""
    import tt_embeddings as E

    fake = 4096
    g = E._geom(2, P, [4, 4, 4], [1, 32, 32, 1])
    gv = E._geom(0, [P, [7, 9, 11]], [4, 4, 4], [1, 32, 32, 1])
    for lib in _libs():
        lib.ttx_tt_expand_supported.argtypes = [ctypes.POINTER(E._Geom)]
        lib.ttx_tt_expand.argtypes = [ctypes.POINTER(E._Geom), i32, i64, i64, vp, vp, vp]
        assert lib.ttx_tt_expand_supported(None) == 0

        def expand(**kw):
            a = dict(g=ctypes.byref(g), table=1, b=40, e=70, cores=(vp * 3)(fake, fake, fake), out=fake)
            a.update(kw)
            return lib.ttx_tt_expand(a["g"], a["table"], a["b"], a["e"], a["cores"], a["out"], None)

        for kw in [dict(g=None), dict(table=-1), dict(table=2), dict(b=-1), dict(b=71), dict(e=445), dict(cores=None), dict(out=None),
                   dict(cores=(vp * 3)(fake, None, fake)), dict(out=fake + 2), dict(cores=(vp * 3)(fake, fake, fake + 1)),
                   dict(g=ctypes.byref(gv), table=2), dict(g=ctypes.byref(gv), table=1, e=7 * 9 * 11 + 1)]:
            assert expand(**kw) == -1 and b"tt_expand" in lib.ttx_last_error(), kw
        for T in (2, 4):
            p, q, r = G.test_shape(T)
            assert expand(g=ctypes.byref(E._geom(1, list(p), list(q), [1] + list(r) + [1])), table=0, b=0, e=1) == -3
        assert expand(b=7, e=7, cores=None, out=None) == 0 and expand(g=ctypes.byref(gv), table=0, b=444, e=444) == 0


def test_expand_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed); the figures are in DESIGN.md 4.22"""
    from test_kernel_resources import resources

    res = resources("ttx_tt_expand.hip")
    assert len(res) == 9 and all("tt_expand_kernel" in k for k in res), sorted(res)
    for k, v in res.items():
        print(k, v)
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0, (k, v)
