"""GPU tests of the pooled one-launch bf16 forward (include/ttx.h "bf16 inference forward, pooled in one launch")
through tt_embeddings.tt_bags_bf16.  Shapes: [4,4,4] / [32,32] the benchmark geometry, one tile everywhere; [3,4,5] / [13,12] q0 does
not divide 16, every rank padded, masked scalar stores; [4,4,8] / [64,64] KB = K2B = 2; [2,4,32] / [16,16] two N tiles in product
2; [8,8,4] / [32,32] four M tiles in product 2.  One batch holds bags of 0, 1, 3, 4, 5, 9 and 33 slots and one with the table's
first and last row and a duplicate index, per table.  Integer cores and weights must give the int64 sum EXACTLY; real cores stay
within the derived bound of tests/bf16b_ref.py against float64 on the same bf16 cores (worst ratio printed: pytest -s)."""
import numpy as np
import pytest
import torch

import bf16_ref as R
import bf16b_ref as RB
import gen_inputs as G
from test_bf16_infer_gpu import P_A, P_B, _int_cores, _pad, _source, t

pytestmark = pytest.mark.gpu

SHAPES = [([4, 4, 4], [32, 32]), ([3, 4, 5], [13, 12]), ([4, 4, 8], [64, 64]), ([2, 4, 32], [16, 16]), ([8, 8, 4], [32, 32])]
LENS, PAD = [0, 1, 3, 4, 5, 9, 33], 3


def _batch(rs, tables, E):
    """per table the bags of LENS and [first row, last row, a duplicate pair]; PAD in front of, inside and as the whole of bags"""
    idx = []
    for _ in range(tables):
        bags = [rs.randint(0, E, size=n) for n in LENS]
        bags[1][:], bags[2][:], bags[4][0], bags[5][4], bags[6][[2, 17, 32]] = PAD, PAD, PAD, PAD, PAD
        idx += bags + [np.array([0, E - 1, 7, 7])]
    off = np.concatenate([[0], np.cumsum([len(b) for b in idx])]).astype(np.int64)
    return np.concatenate(idx).astype(np.int64), off


def _call(E_, tables, p, q, r, packed, idx, off, w=None, pad=None, mean=False):
    return E_.tt_bags_bf16(tables, int(np.prod(q)), p, q, _pad(r), t(idx), t(off), packed, None if w is None else t(w), pad, mean)


@pytest.mark.parametrize("tables", [1, 3])
@pytest.mark.parametrize("q,r", SHAPES)
def test_integer_cores_and_weights_give_the_exact_sums(q, r, tables):
    import tt_embeddings as E_

    p = P_A if tables == 1 else P_B
    cores = _int_cores(11, G.core_shapes(tables, p, q, r))
    packed = E_.pack_cores_bf16m(tables, p, q, _pad(r), [t(c) for c in cores])
    rs = np.random.RandomState(12)
    idx, off = _batch(rs, tables, int(np.prod(p)))
    w = rs.randint(-2, 3, size=idx.size).astype(np.float32)  # (|x_0 w| <= 2 r1 <= 128: exact in bf16)
    for name, kw in (("plain", {}), ("weights", dict(w=w)), ("padding", dict(pad=PAD))):
        got = _call(E_, tables, p, q, r, packed, idx, off, **kw).cpu().numpy()
        want, _ = RB.bags64(cores, p, q, r, tables, idx, off, kw.get("w"), kw.get("pad"))  # (float64: exact on these integers)
        assert np.abs(want).max() < 2 ** 24
        assert np.array_equal(got, want.astype(np.float32)), f"{name}: {int((got != want).sum())} of {want.size} elements differ"


@pytest.mark.parametrize("dist", ["uniform", "signed"])
@pytest.mark.parametrize("q,r", SHAPES)
def test_real_cores_within_the_derived_bound(q, r, dist):
    import tt_embeddings as E_

    for tables, p in ((1, P_A), (3, P_B)):
        cores = [R.to_bf16(c) for c in G.make_cores(41, tables, p, q, r, dist)]
        packed = E_.pack_cores_bf16m(tables, p, q, _pad(r), [t(c) for c in cores])
        rs = np.random.RandomState(42)
        idx, off = _batch(rs, tables, int(np.prod(p)))
        w = rs.uniform(-2, 2, size=idx.size).astype(np.float32)
        forms = (("sum", {}), ("mean", dict(mean=True)), ("weighted", dict(w=w)), ("padded sum", dict(pad=PAD)),
                 ("padded mean", dict(pad=PAD, mean=True)))
        for name, kw in forms:
            out = _call(E_, tables, p, q, r, packed, idx, off, **kw)
            assert torch.equal(_call(E_, tables, p, q, r, packed, idx, off, **kw), out)  # (the same call twice: bit-equal)
            ref, bnd = RB.bags64(cores, p, q, r, tables, idx, off, kw.get("w"), kw.get("pad"), kw.get("mean", False))
            got = out.cpu().numpy()
            err = np.abs(got - ref)  # (float64: ref is)
            ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
            print(f"q={q} r={r} {dist} tables={tables} {name}: worst err / bound {ratio:.5f}, max|out| {np.abs(ref).max():.3e}")
            assert (err <= bnd).all(), f"tables={tables} {name}: worst err / bound {ratio:.3f}"
            assert "pad" not in kw or not (got[1::len(LENS) + 1].any() or got[2::len(LENS) + 1].any())  # (an all-padding bag: zeros)


@pytest.mark.parametrize("kind,tables,mode", [("batched", 3, "sum"), ("bag", 1, "mean"), ("bag", 1, "sum")])
def test_from_module_fused_bags_serves_within_the_bound(kind, tables, mode):
    import ttx_infer

    q, r, p = [3, 4, 5], [13, 12], P_B
    N, L, rs = tables * 4, 6, np.random.RandomState(72)
    idx = rs.randint(0, int(np.prod(p)), size=(N, L)).astype(np.int64)
    idx[1, :2], idx[2, :] = PAD, PAD
    off = np.arange(0, N * L + 1, L)
    w = rs.uniform(-2, 2, size=(N, L)).astype(np.float32)
    for pad in (None, PAD):
        m, E, D = _source(kind, tables, q, r, p, mode, **({} if pad is None else dict(padding_idx=pad)))
        inf = ttx_infer.TTInferenceBag.from_module(m, fused_bags=True)
        assert inf.route == "bf16b" and inf.padding_idx == pad and not list(inf.parameters()) and len(list(inf.buffers())) == 3
        cores = [R.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores]
        calls = [((t(idx),), None)] + ([((t(idx), None, t(w)), w.reshape(-1))] if mode == "sum" else [])
        for args, ww in calls:
            ref, bnd = RB.bags64(cores, p, q, r, tables, idx.reshape(-1), off, ww, pad, mode == "mean")
            out = inf(*args)
            assert tuple(out.shape) == ((N, D) if kind == "bag" else (tables, N // tables, D))
            err = np.abs(out.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
            print(f"{kind} {mode} pad={pad} weights={ww is not None}: worst err / bound {float(np.max(err / np.maximum(bnd, 1e-300))):.5f}")
            assert (err <= bnd).all()
    side = torch.cuda.Stream()  # a captured forward replayed equals eager
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        inf(*args)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        g_out = inf(*args)
    for _ in range(2):
        g_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, out)
