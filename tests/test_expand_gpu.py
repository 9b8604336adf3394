"""GPU tests of the expand kernel and dense_rows (include/ttx.h "dense rows") against the float64 chain product of
the same fp32 cores, within the derived bound (the fp32 term of tests/bf16_ref.py's):

    |err(row[a, b, c])| <= (r1 + r2 + 2) 2^-24 sum_{k1, k2} |c_0[a, k1]| |c_1[k1, (b, k2)]| |c_2[k2, c]|

p = [3, 4, 37]: 444 rows, and 37 leaves a remainder in an i2 tile of any power-of-two width.  Shapes (q, ranks):
  [4,4,4]  / [32,32]     the benchmark's: one N tile, four rows of the table per M tile, 16-byte stores
  [3,4,5]  / [13,12]     nothing a multiple of 4: scalar stores, K padding in both products, q0 q1 = 12 < 16
  [2,2,16] / [16,16]     q0 q1 = 4; one row of the table per M tile
  [4,8,4]  / [64,64]     two N tiles, 16 K blocks
  [8,8,16] / [128,128]   four N tiles, 32 K blocks: the largest instantiation
Worst err / bound printed (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G
from test_bf16_infer_gpu import _pad, dev, t

pytestmark = pytest.mark.gpu

P = [3, 4, 37]
SHAPES = [([4, 4, 4], [32, 32]), ([3, 4, 5], [13, 12]), ([2, 2, 16], [16, 16]), ([4, 8, 4], [64, 64]), ([8, 8, 16], [128, 128])]
RANGES = [(0, 444), (5, 6), (40, 70), (30, 37), (100, 300), (7, 7)]


def _ref(cores, p, q, r, table=0, base=None):
    """-> (rows [prod(p of the table), D] float64, bound) of one table"""
    n = int(np.prod(p if base is None else p[table]))
    A, B, C = R.slices(cores, p, q, r, np.arange(n), np.full(n, table), base=base)
    t2 = np.einsum("nak,nkbj,njc->nabc", np.abs(A), np.abs(B), np.abs(C))
    return R.rows64(A, B, C)[0], ((r[0] + r[1] + 2) * R.U24 * t2).reshape(n, -1)


@functools.lru_cache(maxsize=None)
def _table(i):
    q, r = SHAPES[i]
    cores = G.make_cores(51 + i, 1, P, q, r, "signed")
    return cores, _ref(cores, P, q, r)


def _check(got, ref, bnd, what):
    err = np.abs(got.double().cpu().numpy() - ref)
    ratio = float(np.max(err / np.maximum(bnd, 1e-300))) if err.size else 0.0
    print(f"{what}: worst err / bound {ratio:.4f}")
    assert (err <= bnd).all(), f"{what}: worst err / bound {ratio:.3f}"


@pytest.mark.parametrize("i", range(len(SHAPES)))
def test_ranges_within_the_bound_and_nothing_else_written(i):
    import tt_embeddings as E_

    (q, r), (cores, (ref, bnd)) = SHAPES[i], _table(i)
    D, dc = int(np.prod(q)), [t(c) for c in cores]
    for b, e in RANGES:
        flat = torch.full(((e - b + 2) * D + 1,), float("nan"), device=dev())
        for shift in (0, 1):  # (1: `out` is not 16-byte aligned -- scalar stores whatever q2)
            buf = flat[shift:shift + (e - b + 2) * D].view(e - b + 2, D).fill_(float("nan"))
            out = E_.tt_expand(1, D, P, q, _pad(r), 0, b, e, dc, out=buf[1:e - b + 1])
            assert out.shape == (e - b, D) and torch.isnan(buf[0]).all() and torch.isnan(buf[-1]).all()  # (the guard rows)
            assert not torch.isnan(buf[1:-1]).any()  # (written in place; an empty range has no row to write)
            _check(out, ref[b:e], bnd[b:e], f"q={q} r={r} [{b}, {e}) shift {shift}")
            assert torch.equal(E_.tt_expand(1, D, P, q, _pad(r), 0, b, e, dc), out)  # bit-equal from call to call


def test_tables_var_tables_and_short_tables():
    import tt_embeddings_ops as ops
    import ttx_mixed

    q, r, D = [4, 4, 4], [32, 32], 64
    m = ops.TableBatchedTTEmbeddingBag(3, 400, D, r, P, q, weight_dist="uniform", device=dev())  # (400 < prod(p) = 444)
    pv = [[5, 6, 7], P]
    v = ttx_mixed.VarTableTTEmbeddingBag([200, 444], D, r, pv, q, weight_dist="uniform", device=dev())
    with torch.no_grad():
        for mod, tables, p, seed in ((m, 3, P, 61), (v, 1, [8, 10, 44], 62)):
            for dst, src in zip(mod.tt_cores, G.make_cores(seed, tables, p, q, r, "signed")):
                dst.copy_(t(src))
    ref, bnd = _ref([c.detach().cpu().numpy() for c in m.tt_cores], P, q, r, table=1)
    got = m.dense_rows(table=1)
    assert got.shape == (400, D) and not got.requires_grad
    _check(got, ref[:400], bnd[:400], "table 1 of 3, stop=None")
    _check(m.dense_rows(390, 400, table=1), ref[390:400], bnd[390:400], "table 1 of 3, [390, 400)")
    with pytest.raises(IndexError):
        m.dense_rows(0, 401, table=1)
    base = [[0, 0, 0], pv[0]]
    for k, E in ((0, 200), (1, 444)):
        ref, bnd = _ref([c.detach().cpu().numpy() for c in v.tt_cores], pv, q, r, table=k, base=base)
        _check(v.dense_rows(table=k), ref[:E], bnd[:E], f"VarTable table {k}")
        _check(v.dense_rows(33, 150, table=k), ref[33:150], bnd[33:150], f"VarTable table {k} [33, 150)")


def test_captured_replay_equals_eager():
    import tt_embeddings_ops as ops

    q, r = SHAPES[1]
    m = ops.TTEmbeddingBag(444, 60, r, P, q, weight_dist="uniform", device=dev(), use_cache=False)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, _table(1)[0]):
            dst.copy_(t(src))
    want = m.dense_rows(40, 300)
    _check(want, _table(1)[1][0][40:300], _table(1)[1][1][40:300], "module [40, 300)")
    out = torch.empty_like(want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m.dense_rows(40, 300, out=out)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        m.dense_rows(40, 300, out=out)
    for _ in range(3):
        out.fill_(float("nan"))  # (a kernel, not a memset node: outside the graph)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.parametrize("T", [2, 4])
def test_fallback_equals_full_weight(T):
    import tt_embeddings as E_
    import tt_embeddings_ops as ops

    p, q, r = G.test_shape(T)
    E, D = int(np.prod(p)), int(np.prod(q))
    m = ops.TableBatchedTTEmbeddingBag(2, E, D, list(r), list(p), list(q), weight_dist="uniform", device=dev())
    assert not E_.tt_expand_supported(2, p, q, _pad(r))
    m._DENSE_ROWS_BLOCK = 64  # (several blocks at this size)
    full = m.full_weight(1)
    for start, stop in ((0, None), (E // 3, min(E, E // 3 + 100))):
        got, want = m.dense_rows(start, stop, table=1), full[start:stop]
        assert got.shape == want.shape
        assert ((got - want).abs() <= 2e-6 * want.abs().max() + 1e-5 * want.abs()).all()  # (the fp32 route's tolerance: smoke())


def test_argument_errors_and_the_live_cache():
    import tt_embeddings as E_
    import tt_embeddings_ops as ops

    q, r = SHAPES[0]
    dc = [t(c) for c in _table(0)[0]]
    for table, b, e in ((1, 0, 4), (-1, 0, 4), (0, -1, 4), (0, 5, 4), (0, 0, 445)):
        with pytest.raises(RuntimeError, match="tt_expand"):
            E_.tt_expand(1, 64, P, q, _pad(r), table, b, e, dc)
    with pytest.raises(RuntimeError, match="out must be"):
        E_.tt_expand(1, 64, P, q, _pad(r), 0, 0, 4, dc, out=torch.empty(5, 64, device=dev()))
    m = ops.TTEmbeddingBag(444, 64, r, P, q, weight_dist="uniform", device=dev(), use_cache=True, cache_size=16, hashtbl_size=512)
    assert m.dense_rows(5, 9).shape == (4, 64)  # (warm-up: the cache holds nothing yet)
    m(t(np.arange(8, dtype=np.int64)), t(np.array([0, 4, 8], dtype=np.int64)))
    m.cache_populate()
    with pytest.raises(ValueError, match="row cache is live"):
        m.dense_rows(5, 9)
