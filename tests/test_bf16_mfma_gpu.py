"""GPU tests of the MFMA-tail bf16 inference forward (include/ttx.h "bf16 inference forward, MFMA tail"), at the
smallest shapes that reach each way the kernel can go wrong:

  [2,2,16]   / [16,16]    one K block in each product; a lookup's 4 rows fill a quarter of a product-2 tile; largest SC (32)
  [8,8,16]   / [32,32]    D = 1024's default factoring; two lookups per product-1 tile; full product-2 tiles
  [3,5,10]   / [40,33]    q0 does not divide 16; q0 q1 = 15; q2 % 4 != 0 (scalar stores, masked c); r1 and r2 padded; K2p = 64
                          with only 48 columns written (the zeroed pad)
  [4,4,32]   / [64,64]    Q2P = 32 (two M tiles); KB = K2B = 2
  [16,16,16] / [64,128]   D = 4096's default factoring; K2B = 4; SC = 1; an X above 64 KiB

Integer cores must give the int64 chain product EXACTLY (|x_0| <= 128 is exact in bf16, |row| <= 16384 < 2^24); real cores stay
within the derived bound of tests/bf16_ref.py against float64 on the same bf16 cores -- this kernel rounds x_0 to bf16, so the
bound's 2^-8 term is in use (worst ratio printed: pytest -s, profiles/r21_bf16_mfma.md)."""
import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G
from test_bf16_infer_gpu import P_A, P_B, P_TABLES, _int_cores, _one_slice, _pad, _ragged, _source, t

pytestmark = pytest.mark.gpu

SHAPES = [([2, 2, 16], [16, 16]), ([8, 8, 16], [32, 32]), ([3, 5, 10], [40, 33]), ([4, 4, 32], [64, 64]), ([16, 16, 16], [64, 128])]
SC = [32, 8, 21, 16, 1]  # lookups of a pass (64 // q0, fewer where x_0 passes 80 KiB: the last shape, 68 KiB each)


def _rows(E_, tables, p, q, r, cores, idx, tab):
    packed = E_.pack_cores_bf16m(tables, p, q, _pad(r), [t(c) for c in cores])
    return E_.tt_rows_bf16m(tables, int(np.prod(q)), p, q, _pad(r), t(idx), t(tab), packed).cpu().numpy()


@pytest.mark.parametrize("q,r,sc", [(q, r, sc) for (q, r), sc in zip(SHAPES, SC)])
def test_integer_cores_give_the_exact_rows(q, r, sc):
    import tt_embeddings as E_

    rs = np.random.RandomState(12)
    mc = E_.debug_plan_layout(1, P_A, q, _pad(r), 64)["MC"]
    mc = E_.debug_plan_layout(1, P_A, q, _pad(r), mc + 1)["MC"]
    assert mc >= 1
    Ea, Eb = int(np.prod(P_A)), int(np.prod(P_B))
    batches = [(1, P_A, rs.randint(0, Ea, size=1)), (1, P_A, rs.randint(0, Ea, size=7))]
    batches += [(1, P_A, _one_slice(rs, P_A, n, 2)) for n in (sc - 1, sc, sc + 1, mc + 1) if n > 0]
    dup = rs.randint(0, Eb, size=300)
    dup[100:200] = dup[:100]
    batches.append((3, P_B, dup))
    for tables, p, idx in batches:
        cores = _int_cores(11, G.core_shapes(tables, p, q, r))
        idx = idx.astype(np.int64)
        tab = rs.randint(0, tables, size=idx.size).astype(np.int64)
        got = _rows(E_, tables, p, q, r, cores, idx, tab)
        key, inv = np.unique(tab * int(np.prod(p)) + idx, return_inverse=True)  # (each distinct lookup contracted once)
        A, B, C = R.slices(cores, p, q, r, key % int(np.prod(p)), key // int(np.prod(p)))  # (float64: exact on these integers)
        x0 = np.matmul(A, B.reshape(key.size, r[0], -1)).reshape(key.size, -1, r[1])
        want = np.matmul(x0, C).reshape(key.size, -1)[inv]
        assert np.abs(x0).max() <= 128 and np.abs(want).max() <= 16384
        assert np.array_equal(got, want.astype(np.float32)), \
            f"tables={tables} n={idx.size}: {int((got != want).sum())} of {want.size} elements differ"


@pytest.mark.parametrize("dist", ["uniform", "signed"])
@pytest.mark.parametrize("q,r", SHAPES)
def test_real_cores_within_the_derived_bound(q, r, dist):
    import tt_embeddings as E_

    base = [[sum(row[k] for row in P_TABLES[:j]) for k in range(3)] for j in range(len(P_TABLES))]
    cases = [(1, P_A, None), (3, P_B, None)]
    if r == [40, 33]:  # per-table row factors, once
        cases.append((0, P_TABLES, base))
    for tables, p, pbase in cases:
        n = 64
        rs = np.random.RandomState(42)
        tab = np.sort(rs.randint(0, max(tables, 1) if pbase is None else len(p), size=n)).astype(np.int64)
        if pbase is None:
            cores = [R.to_bf16(c) for c in G.make_cores(41, tables, p, q, r, dist)]
            idx = rs.randint(0, int(np.prod(p)), size=n).astype(np.int64)
        else:
            cores = [R.to_bf16(c) for c in G.make_cores(41, 1, [sum(row[k] for row in p) for k in range(3)], q, r, dist)]
            idx = np.array([rs.randint(0, int(np.prod(p[k]))) for k in tab], dtype=np.int64)
        got = _rows(E_, tables, p, q, r, cores, idx, tab).astype(np.float64)
        ref, bnd = R.rows64(*R.slices(cores, p, q, r, idx, tab, base=pbase))
        err = np.abs(got - ref)
        ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
        print(f"q={q} r={r} {dist} tables={tables}: worst err / bound {ratio:.5f}, max|row| {np.abs(ref).max():.3e}")
        assert (err <= bnd).all(), f"tables={tables}: worst err / bound {ratio:.3f}"


@pytest.mark.parametrize("q,r", SHAPES[1:4])
def test_pack_is_bit_equal_to_the_torch_pack(q, r):
    import tt_embeddings as E_
    import ttx_infer

    cores = G.make_cores(31, 2, P_A, q, r, "signed")
    got = E_.pack_cores_bf16m(2, P_A, q, _pad(r), [t(c) for c in cores])
    want = ttx_infer.pack_cores_torch([torch.from_numpy(c) for c in cores], q, _pad(r), mfma_tail=True)
    for g, w in zip(got, want):
        assert g.dtype == torch.bfloat16 and torch.equal(g.cpu().view(torch.int16), w.view(torch.int16))


@pytest.mark.parametrize("kind,tables,mode", [("batched", 3, "sum"), ("bag", 1, "mean"), ("embedding", 1, "sum")])
def test_from_module_mfma_tail_serves_within_the_pooled_bound(kind, tables, mode):
    import ttx_infer

    q, r, p = [8, 8, 16], [32, 32], P_B
    m, E, D = _source(kind, tables, q, r, p, mode)
    assert ttx_infer.TTInferenceBag.from_module(m).route == "fp32"  # (the default stays)
    assert ttx_infer.TTInferenceBag.from_module(m, wide=True).route == "fp32"
    inf = ttx_infer.TTInferenceBag.from_module(m, mfma_tail=True)
    assert inf.route == "bf16m" and not list(inf.parameters()) and len(list(inf.buffers())) == 3
    cores = [R.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores]
    rs = np.random.RandomState(72)
    if kind == "embedding":
        idx = rs.randint(0, E, size=(4, 9)).astype(np.int64)
        args = (t(idx),)
        ref, bnd = R.rows64(*R.slices(cores, p, q, r, idx.reshape(-1), np.zeros(idx.size, np.int64)))
    else:
        idx, off = _ragged(rs, tables * 9, E)
        args = (t(idx), t(off))
        tab = np.repeat(np.arange(tables * 9) // 9, np.diff(off))
        ref, bnd = R.pool64(*R.rows64(*R.slices(cores, p, q, r, idx, tab)), off, mean=mode == "mean")
    out = inf(*args)
    err = np.abs(out.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
    print(f"{kind} tables={tables} {mode}: worst err / pooled bound {float(np.max(err / np.maximum(bnd, 1e-300))):.5f}")
    assert (err <= bnd).all() and torch.equal(inf(*args), out)
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
