"""The four-core bf16 inference forward without a GPU: the shapes it takes, the torch pack / unpack round trip of
its layout, TTInferenceBag.from_module(m, four_cores=True) on CPU tensors (the torch-op chain product) within the derived bound
of tests/bf16q_ref.py, and that bound's own check of itself."""
import numpy as np
import pytest
import torch

import bf16q_ref as Q
import gen_inputs as G
from test_bf16_infer_cpu import _bags, _module, ops  # noqa: F401  (ops: the oracle-engine fixture)

P4 = [3, 4, 5, 6]


def test_supported_shapes():
    import tt_embeddings as E

    for q, r in Q.SHAPES:
        for tables, p in ((1, P4), (3, [4, 5, 6, 7]), (0, [[3, 4, 5, 6], [4, 5, 6, 7], [2, 3, 2, 3]])):
            assert E.tt_rows_bf16q_supported(tables, p, q, [1] + r + [1]), (q, r)
    assert not E.tt_rows_bf16q_supported(1, [5, 6, 7], [4, 4, 4], [1, 32, 32, 1])  # T = 3
    for r in ([65, 32, 32], [32, 65, 32], [32, 32, 65]):
        assert not E.tt_rows_bf16q_supported(1, P4, [4, 4, 4, 4], [1] + r + [1])
    assert not E.tt_rows_bf16q_supported(1, P4, [4, 4, 3, 11], [1, 32, 32, 32, 1])  # q2 q3 = 33
    assert E.tt_rows_bf16q_supported(1, P4, [4, 4, 2, 16], [1, 32, 32, 32, 1])
    assert not E.tt_rows_bf16q_supported(1, P4, [4, 4, 1, 17], [1, 32, 32, 32, 1])  # q3 beyond one MFMA tile
    g = E._geom(1, P4, [3, 5, 2, 5], [1, 40, 33, 24, 1])  # K1p = 64, N1p = 176, K3p = 32
    assert [E.lib().ttx_tt_pack_bf16q_elems(E.C.byref(g), t) for t in (0, 1, 2, 3, 4, -1)] == \
        [3 * 3 * 64, 4 * 176 * 64, 5 * 66 * 32, 6 * 16 * 32, 0, 0]


@pytest.mark.parametrize("q,r", [Q.SHAPES[2], Q.SHAPES[4]])
def test_packed_layout_round_trip_with_torch_ops(q, r):
    import ttx_infer

    rr = [1] + r + [1]
    cores = [torch.from_numpy(c) for c in G.make_cores(9, 2, P4, q, r, "signed")]
    pk = ttx_infer.pack_cores_torch(cores, q, rr)
    K3p = -(-r[2] // 32) * 32
    assert [x.numel() for x in pk[2:]] == [2 * P4[2] * r[1] * q[2] * K3p, 2 * P4[3] * 16 * K3p]
    c2 = cores[2].view(2 * P4[2], r[1], q[2], r[2]).to(torch.bfloat16)
    c3 = cores[3].view(2 * P4[3], r[2], q[3]).to(torch.bfloat16)
    p2, p3 = pk[2].view(2 * P4[2], r[1] * q[2], K3p), pk[3].view(2 * P4[3], 16, K3p)
    assert p2[7, 5 * q[2] + 1, 9] == c2[7, 5, 1, 9] and not p2[:, :, r[2]:].any()
    assert p3[8, 3, 11] == c3[8, 11, 3] and not p3[:, q[3]:].any() and not p3[:, :, r[2]:].any()
    for b, c in zip(ttx_infer.unpack_cores_torch(pk, q, rr), cores):
        assert torch.equal(b, c.view(-1, c.size(-1)).to(torch.bfloat16).float())


@pytest.mark.parametrize("q,r", [Q.SHAPES[1], Q.SHAPES[2]])
def test_from_module_four_cores_on_cpu_tensors(ops, q, r):  # noqa: F811
    import ttx_infer

    for kind, tables, mode in (("batched", 3, "mean"), ("bag", 1, "sum")):
        m, E, D = _module(ops, kind, tables, q, r, p=P4, mode=mode)
        assert ttx_infer.TTInferenceBag.from_module(m).route == "fp32"
        inf = ttx_infer.TTInferenceBag.from_module(m, four_cores=True)
        assert inf.route == "bf16q" and not list(inf.parameters())
        assert len(list(inf.buffers())) == 4 and all(b.dtype == torch.bfloat16 for b in inf.buffers())
        cores = [Q.to_bf16(c.detach().numpy()) for c in m.tt_cores]
        idx, off = _bags(np.random.RandomState(7), tables, 6, E)
        out = inf(torch.from_numpy(idx), torch.from_numpy(off))
        tab = np.repeat(np.arange(tables * 6) // 6, np.diff(off))
        ref, bnd = Q.pool64(*Q.rows64(*Q.slices(cores, P4, q, r, idx, tab)), off, mean=mode == "mean")
        err = np.abs(out.numpy().astype(np.float64).reshape(ref.shape) - ref)
        assert (err <= bnd).all(), f"{kind} {mode}: worst err / bound {np.max(err / np.maximum(bnd, 1e-300)):.3f}"
    # a three-core geometry keeps its route with the flag
    assert ttx_infer.TTInferenceBag.from_module(_module(ops, "bag", 1, [2, 2, 4], [16, 16])[0], four_cores=True).route == "bf16"


def test_bound_catches_a_dropped_term():
    """the bound is tight enough to see one missing k2 term on most elements (bf16_ref's own check, carried to four cores)"""
    q, r = [4, 4, 4, 4], [32, 32, 32]
    for dist in ("uniform", "signed"):
        cores = [Q.to_bf16(c) for c in G.make_cores(5, 1, P4, q, r, dist)]
        idx = np.random.RandomState(1).randint(0, int(np.prod(P4)), size=40)
        A, B, C, Dm = Q.slices(cores, P4, q, r, idx, np.zeros(40, np.int64))
        ref, bnd = Q.rows64(A, B, C, Dm)
        C2 = C.copy()
        C2[:, 5] = 0.0  # drop k2 = 5
        assert (np.abs(Q.rows64(A, B, C2, Dm)[0] - ref) > bnd).mean() > 0.5
