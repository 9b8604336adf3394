"""GPU tests of the four-core bf16 inference forward (include/ttx.h "bf16 inference forward, four cores"), at
the smallest shapes that reach each way the kernel can go wrong:

  [2,2,2,2] / [16,16,16]   q0 q1 = 4: a quarter tile; q2 q3 = 4: masked (c, d); largest SC (32); one K block everywhere
  [4,4,4,4] / [32,32,32]   D = 256's default; full tiles; 16-byte stores
  [3,5,2,5] / [40,33,24]   q0 does not divide 16; q2 q3 = 10: scalar stores; every rank padded; K2p = 64 with 48 columns written
                           (the zeroed pads of X and Y)
  [4,4,4,8] / [64,64,64]   Q23P = 32 (two M tiles); two K blocks in all three products
  [2,4,4,4] / [32,64,16]   KB, K2B, K3B differ; D = 128's default factoring

Integer cores must give the int64 chain product EXACTLY (|x_0|, |M| <= 64 are exact in bf16, |row| <= 64^3 < 2^24); real cores
stay within the derived bound of tests/bf16q_ref.py against float64 on the same bf16 cores (worst ratio printed: pytest -s,
profiles/r24_bf16_quad.md)."""
import numpy as np
import pytest
import torch

import bf16q_ref as Q
import gen_inputs as G
from test_bf16_infer_gpu import _int_cores, _pad, _ragged, _source, t

pytestmark = pytest.mark.gpu

P_A, P_B = [3, 4, 5, 6], [4, 5, 6, 7]
P_TABLES = [[3, 4, 5, 6], [4, 5, 6, 7], [2, 3, 2, 3]]
SC = [32, 16, 17, 11, 22]  # lookups of a pass (64 // q0, fewer where x_0 and M of the pass exceed 80 KiB)


def _rows(E_, tables, p, q, r, cores, idx, tab):
    packed = E_.pack_cores_bf16q(tables, p, q, _pad(r), [t(c) for c in cores])
    return E_.tt_rows_bf16q(tables, int(np.prod(q)), p, q, _pad(r), t(idx), t(tab), packed).cpu().numpy()


def _one_slice(rs, p, n, i1):
    """n lookups that share core 1's slice i1"""
    return ((rs.randint(0, p[0], size=n) * p[1] + i1) * p[2] + rs.randint(0, p[2], size=n)) * p[3] + rs.randint(0, p[3], size=n)


@pytest.mark.parametrize("q,r,sc", [(q, r, sc) for (q, r), sc in zip(Q.SHAPES, SC)])
def test_integer_cores_give_the_exact_rows(q, r, sc):
    import tt_embeddings as E_

    rs = np.random.RandomState(12)
    mc = E_.debug_plan_layout(1, P_A, q, _pad(r), 64)["MC"]
    mc = E_.debug_plan_layout(1, P_A, q, _pad(r), mc + 1)["MC"]
    assert mc >= 1
    Ea, Eb = int(np.prod(P_A)), int(np.prod(P_B))
    batches = [(1, P_A, rs.randint(0, Ea, size=1)), (1, P_A, rs.randint(0, Ea, size=7))]
    batches += [(1, P_A, _one_slice(rs, P_A, n, 2)) for n in (sc - 1, sc, sc + 1, mc + 1)]
    dup = rs.randint(0, Eb, size=300)
    dup[100:200] = dup[:100]
    batches.append((3, P_B, dup))
    for tables, p, idx in batches:
        cores = _int_cores(11, G.core_shapes(tables, p, q, r))
        idx = idx.astype(np.int64)
        tab = rs.randint(0, tables, size=idx.size).astype(np.int64)
        got = _rows(E_, tables, p, q, r, cores, idx, tab)
        x0, M, want = Q.chain(*[a.astype(np.int64) for a in Q.slices(cores, p, q, r, idx, tab)])
        assert np.abs(x0).max() <= 64 and np.abs(M).max() <= 64 and np.abs(want).max() < 2 ** 24
        want = want.reshape(idx.size, -1)
        assert np.array_equal(got, want.astype(np.float32)), \
            f"tables={tables} n={idx.size}: {int((got != want).sum())} of {want.size} elements differ"


@pytest.mark.parametrize("dist", ["uniform", "signed"])
@pytest.mark.parametrize("q,r", Q.SHAPES)
def test_real_cores_within_the_derived_bound(q, r, dist):
    import tt_embeddings as E_

    base = [[sum(row[k] for row in P_TABLES[:j]) for k in range(4)] for j in range(len(P_TABLES))]
    cases = [(1, P_A, None), (3, P_B, None)]
    if r == [40, 33, 24]:  # per-table row factors, once
        cases.append((0, P_TABLES, base))
    for tables, p, pbase in cases:
        n = 64
        rs = np.random.RandomState(42)
        tab = np.sort(rs.randint(0, max(tables, 1) if pbase is None else len(p), size=n)).astype(np.int64)
        if pbase is None:
            cores = [Q.to_bf16(c) for c in G.make_cores(41, tables, p, q, r, dist)]
            idx = rs.randint(0, int(np.prod(p)), size=n).astype(np.int64)
        else:
            cores = [Q.to_bf16(c) for c in G.make_cores(41, 1, [sum(row[k] for row in p) for k in range(4)], q, r, dist)]
            idx = np.array([rs.randint(0, int(np.prod(p[k]))) for k in tab], dtype=np.int64)
        got = _rows(E_, tables, p, q, r, cores, idx, tab).astype(np.float64)
        ref, bnd = Q.rows64(*Q.slices(cores, p, q, r, idx, tab, base=pbase))
        err = np.abs(got - ref)
        ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
        print(f"q={q} r={r} {dist} tables={tables}: worst err / bound {ratio:.5f}, max|row| {np.abs(ref).max():.3e}")
        assert (err <= bnd).all(), f"tables={tables}: worst err / bound {ratio:.3f}"


@pytest.mark.parametrize("q,r", Q.SHAPES[1:4])
def test_pack_is_bit_equal_to_the_torch_pack(q, r):
    import tt_embeddings as E_
    import ttx_infer

    cores = G.make_cores(31, 2, P_A, q, r, "signed")
    got = E_.pack_cores_bf16q(2, P_A, q, _pad(r), [t(c) for c in cores])
    want = ttx_infer.pack_cores_torch([torch.from_numpy(c) for c in cores], q, _pad(r))
    assert len(got) == len(want) == 4
    for g, w in zip(got, want):
        assert g.dtype == torch.bfloat16 and torch.equal(g.cpu().view(torch.int16), w.view(torch.int16))


@pytest.mark.parametrize("kind,tables,mode", [("batched", 3, "sum"), ("bag", 1, "mean"), ("embedding", 1, "sum")])
def test_from_module_four_cores_serves_within_the_pooled_bound(kind, tables, mode):
    import ttx_infer

    q, r, p = [4, 4, 4, 4], [32, 32, 32], P_B
    m, E, D = _source(kind, tables, q, r, p, mode)
    assert ttx_infer.TTInferenceBag.from_module(m).route == "fp32"  # (the default stays)
    inf = ttx_infer.TTInferenceBag.from_module(m, four_cores=True)
    assert inf.route == "bf16q" and not list(inf.parameters()) and len(list(inf.buffers())) == 4
    cores = [Q.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores]
    rs = np.random.RandomState(72)
    if kind == "embedding":
        idx = rs.randint(0, E, size=36).astype(np.int64)
        off = np.arange(37, dtype=np.int64)  # (every position a bag of one slot)
        args = (t(idx.reshape(4, 9)),)
    else:
        idx, off = _ragged(rs, tables * 9, E)
        args = (t(idx), t(off))
    tab = np.repeat(np.arange(len(off) - 1) // ((len(off) - 1) // tables), np.diff(off))
    rows, rbnd = Q.rows64(*Q.slices(cores, p, q, r, idx, tab))
    pool = (lambda rw, b: (rw, b)) if kind == "embedding" else (lambda rw, b: Q.pool64(rw, b, off, mean=mode == "mean"))
    ref, bnd = pool(rows, rbnd)
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
    # a hot row table on the route: a hit is its computed row rounded once more to bf16 (relative 2^-9 of |row| + bound)
    keys = np.unique(tab * E + idx)[::2]
    hot = [t(keys[keys // E == k] % E) for k in range(tables)]
    served = ttx_infer.TTInferenceBag.from_module(m, four_cores=True, hot_indices=hot if kind == "batched" else hot[0])
    assert served.route == "bf16q" and served.hot_rows_count == keys.size > 0
    hit = np.isin(tab * E + idx, keys)
    hbnd = rbnd + hit[:, None] * 2.0 ** -9 * (np.abs(rows) + rbnd)
    ref, bnd = pool(rows, hbnd)
    err = np.abs(served(*args).cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
    print(f"{kind} hot rows {keys.size}: worst err / pooled bound {float(np.max(err / np.maximum(bnd, 1e-300))):.5f}")
    assert hit.any() and not hit.all() and (err <= bnd).all()
