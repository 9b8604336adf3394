"""GPU tests of the bf16 inference forward (include/ttx.h "bf16 inference forward").

  exact integers   cores drawn from {-1, 0, 1}: every product and sum of the chain is an integer below 2^24 (|x_0| <= 64,
                   |row| <= 4096), exact in bf16 and in fp32 -- the rows must EQUAL the int64 chain product.  A swapped row /
                   column or a permuted k order of the packed layout cannot pass.
  the pack         bit for bit tensor.to(torch.bfloat16), through the packed layout rebuilt with torch ops, and a one-hot probe
                   through the rows kernel.
  real cores       against the float64 chain product on the same bf16 cores within the DERIVED bound of tests/bf16_ref.py; the
                   worst ratio is printed (pytest -s; profiles/r19_bf16_forward.md holds the recorded figures).
  bag_sum_pool     bit-equal to a sequential float32 sum in index order.
  modules          TTInferenceBag.from_module on the three classes; the fp32 fall-back bit-equal to the source's own forward on
                   the rounded cores."""
import numpy as np
import pytest
import torch

import bf16_ref as R
import gen_inputs as G

pytestmark = pytest.mark.gpu

P_A, P_B = [5, 6, 7], [7, 9, 11]
P_TABLES = [[5, 6, 7], [7, 9, 11], [2, 3, 4]]


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _pad(r):
    return [1] + list(r) + [1]


def _int_cores(seed, shapes):
    rs = np.random.RandomState(seed)
    return [rs.choice(np.array([-1.0, 0.0, 1.0], dtype=np.float32), size=s, p=[0.2, 0.45, 0.35]) for s in shapes]


def _rows(E_, tables, p, q, r, cores, idx, tab, plan=None):
    packed = E_.pack_cores_bf16(tables, p, q, _pad(r), [t(c) for c in cores])
    return E_.tt_rows_bf16(tables, int(np.prod(q)), p, q, _pad(r), t(idx), None if tab is None else t(tab), packed, plan)


def _one_slice(rs, p, n, i1):
    """n lookups that share core 1's slice i1"""
    return (rs.randint(0, p[0], size=n) * p[1] + i1) * p[2] + rs.randint(0, p[2], size=n)


# -------------------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("tables", [1, 3])
@pytest.mark.parametrize("q,r", R.SHAPES)
def test_integer_cores_give_the_exact_rows(q, r, tables):
    import tt_embeddings as E_

    p = P_A if tables == 1 else P_B
    cores = _int_cores(11, G.core_shapes(tables, p, q, r))
    packed = E_.pack_cores_bf16(tables, p, q, _pad(r), [t(c) for c in cores])
    D, Ep = int(np.prod(q)), int(np.prod(p))
    rs = np.random.RandomState(12)
    mc = E_.debug_plan_layout(tables, p, q, _pad(r), 64)["MC"]
    assert mc >= 1
    batches = {"1": rs.randint(0, Ep, size=1), "7": rs.randint(0, Ep, size=7)}
    for d in (-1, 0, 1):
        n = max(1, mc + d)
        mcn = E_.debug_plan_layout(tables, p, q, _pad(r), n)["MC"]
        batches[f"MC{d:+d}"] = _one_slice(rs, p, max(1, mcn + d), 2)
    big = 2 * E_.debug_plan_layout(tables, p, q, _pad(r), 2 * mc + 40)["MC"] + 5
    batches[">2MC beside empty slices"] = np.concatenate([_one_slice(rs, p, big, 1), _one_slice(rs, p, 3, p[1] - 1)])
    dup = rs.randint(0, Ep, size=300)
    dup[100:200] = dup[:100]
    batches["300 with duplicates"] = dup
    for name, idx in batches.items():
        idx = idx.astype(np.int64)
        tab = rs.randint(0, tables, size=idx.size).astype(np.int64)
        tab[:] = np.sort(tab) if name != "300 with duplicates" else tab
        if name.startswith("MC") or name.startswith(">"):
            tab[:] = tables - 1  # (one pivot slice: one table)
        got = E_.tt_rows_bf16(tables, D, p, q, _pad(r), t(idx), t(tab), packed).cpu().numpy()
        A, B, C = R.slices(cores, p, q, r, idx, tab)
        want = np.einsum("nabj,njc->nabc", np.einsum("nak,nkbj->nabj", A.astype(np.int64), B.astype(np.int64)),
                         C.astype(np.int64)).reshape(idx.size, D)
        assert np.abs(want).max() <= 4096
        assert np.array_equal(got.astype(np.int64), want) and np.array_equal(got, want.astype(np.float32)), \
            f"{name}: {int((got != want).sum())} of {want.size} elements differ"


def test_integer_cores_with_per_table_row_factors():
    import tt_embeddings as E_

    q, r = [4, 4, 4], [32, 32]
    psum = [sum(row[k] for row in P_TABLES) for k in range(3)]
    rr = _pad(r)
    cores = _int_cores(21, [(1, psum[k], rr[k] * q[k] * rr[k + 1]) for k in range(3)])
    base = [[sum(row[k] for row in P_TABLES[:j]) for k in range(3)] for j in range(len(P_TABLES))]
    rs = np.random.RandomState(22)
    tab = np.sort(rs.randint(0, 3, size=200)).astype(np.int64)
    idx = np.array([rs.randint(0, int(np.prod(P_TABLES[k]))) for k in tab], dtype=np.int64)
    assert E_.tt_rows_bf16_supported(0, P_TABLES, q, rr)
    got = _rows(E_, 0, P_TABLES, q, r, cores, idx, tab).cpu().numpy()
    A, B, C = R.slices(cores, P_TABLES, q, r, idx, tab, base=base)
    want = np.einsum("nabj,njc->nabc", np.einsum("nak,nkbj->nabj", A.astype(np.int64), B.astype(np.int64)),
                     C.astype(np.int64)).reshape(idx.size, -1)
    assert np.array_equal(got, want.astype(np.float32))


# --------------------------------------------------------------------------------------------------------------- the pack
SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8),
            -(1.0 + 3 * 2.0 ** -8), -1.0 - 2.0 ** -8 - 2.0 ** -20, 1e-40, -1e-40, 2.0 ** -149, 3.4028234663852886e38,
            -3.4028234663852886e38, 3.3895313892515355e38, float("inf"), float("-inf"), 0.0, -0.0, 1.0, 0.1, -2.5e-7]


@pytest.mark.parametrize("q,r", [R.SHAPES[1], R.SHAPES[2], R.SHAPES[4]])
def test_pack_is_torch_bf16_in_the_documented_layout(q, r):
    """ttx_tt_pack_bf16 against the layout of ttx.h rebuilt with torch ops (ttx_infer.pack_cores_torch): random values, ties,
    subnormals, the largest finite value, Inf and NaN, bit for bit"""
    import tt_embeddings as E_
    import ttx_infer

    tables = 2
    cores = G.make_cores(31, tables, P_A, q, r, "signed")
    rs = np.random.RandomState(32)
    for c in cores:
        flat = c.reshape(-1)
        pos = rs.choice(flat.size, size=3 * len(SPECIALS) + 3, replace=False)
        flat[pos[:3 * len(SPECIALS)]] = np.array(SPECIALS * 3, dtype=np.float32)
        flat[pos[-3:]] = np.float32("nan")
        ties = rs.choice(flat.size, size=flat.size // 8, replace=False)  # exact ties: the 16 dropped bits are 0x8000
        flat[ties] = ((flat[ties].view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)).view(np.float32)
    got = E_.pack_cores_bf16(tables, P_A, q, _pad(r), [t(c) for c in cores])
    want = ttx_infer.pack_cores_torch([torch.from_numpy(c) for c in cores], q, _pad(r))
    for k in range(3):
        assert got[k].dtype == torch.bfloat16 and got[k].numel() == want[k].numel()
        g, w = got[k].cpu(), want[k]
        # (a NaN stays a NaN; WHICH NaN torch writes depends on its conversion path -- 0x7FC0 scalar, 0xFFFF vectorised -- so
        #  NaNs are compared as NaNs, everything else bit for bit; the library writes 0x7FC0)
        nan = torch.isnan(w.float())
        assert torch.equal(torch.isnan(g.float()), nan) and int(nan.sum()) >= 3, f"core {k}: NaN positions"
        assert (g.view(torch.int16)[torch.isnan(g.float())] == 0x7FC0).all()
        bad = (g.view(torch.int16) != w.view(torch.int16)) & ~nan
        assert not bad.any(), f"core {k}: {int(bad.sum())} differ, first: got {float(g[bad][0])!r} want {float(w[bad][0])!r}"


@pytest.mark.parametrize("v", SPECIALS[:15])
def test_one_hot_probe_through_the_rows_kernel(v):
    """one value v in a core-0 slice, ones at the matching positions of cores 1 and 2: row[0] = bf16(v)"""
    import tt_embeddings as E_

    q, r, p = [2, 2, 4], [16, 16], P_A
    want = torch.tensor(v, dtype=torch.float32).to(torch.bfloat16).float()
    cores = [np.zeros(s, dtype=np.float32) for s in G.core_shapes(1, p, q, r)]
    cores[0].reshape(p[0], q[0], r[0])[1, 0, 3] = v
    c1, c2 = cores[1].reshape(p[1], r[0], q[1], r[1]), cores[2].reshape(p[2], r[1], q[2])
    if torch.isinf(want):  # (0 * Inf is NaN in any arithmetic: every term of row[0] carries the value)
        c1[2, 3, 0, :] = 1.0
        c2[4, :, 0] = 1.0
    else:
        c1[2, 3, 0, 5] = 1.0
        c2[4, 5, 0] = 1.0
    idx = np.array([(1 * p[1] + 2) * p[2] + 4], dtype=np.int64)
    got = _rows(E_, 1, p, q, r, cores, idx, np.zeros(1, np.int64)).cpu()
    assert got[0, 0].view(torch.int32) == want.view(torch.int32), (v, float(got[0, 0]), float(want))


# ------------------------------------------------------------------------------------------------- real cores: the bound
@pytest.mark.parametrize("dist", ["uniform", "signed"])
@pytest.mark.parametrize("q,r", R.SHAPES)
def test_real_cores_within_the_derived_bound(q, r, dist):
    import tt_embeddings as E_

    worst = 0.0
    for tables, p in ((1, P_A), (3, P_B)):
        cores = [R.to_bf16(c) for c in G.make_cores(41, tables, p, q, r, dist)]
        rs = np.random.RandomState(42)
        idx = rs.randint(0, int(np.prod(p)), size=400).astype(np.int64)
        tab = np.sort(rs.randint(0, tables, size=400)).astype(np.int64)
        got = _rows(E_, tables, p, q, r, cores, idx, tab).cpu().numpy().astype(np.float64)
        ref, bnd = R.rows64(*R.slices(cores, p, q, r, idx, tab))
        err = np.abs(got - ref)
        ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
        print(f"q={q} r={r} {dist} tables={tables}: worst err / bound {ratio:.5f}, max|row| {np.abs(ref).max():.3e}")
        assert (err <= bnd).all(), f"tables={tables}: worst err / bound {ratio:.3f}"
        worst = max(worst, ratio)
    print(f"q={q} r={r} {dist}: WORST err / bound {worst:.5f}")


# -------------------------------------------------------------------------------------------------- plan and determinism
def test_plan_handed_in_two_runs_and_a_captured_call():
    import tt_embeddings as E_

    q, r, tables, p = [4, 4, 8], [64, 64], 3, P_B
    D = int(np.prod(q))
    cores = [R.to_bf16(c) for c in G.make_cores(51, tables, p, q, r, "signed")]
    packed = E_.pack_cores_bf16(tables, p, q, _pad(r), [t(c) for c in cores])
    rs = np.random.RandomState(52)
    B = 40
    lens = rs.randint(0, 7, size=tables * B)
    off = t(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
    idx = t(rs.randint(0, int(np.prod(p)), size=int(lens.sum())).astype(np.int64))
    rowidx, tab, plan_bags = E_.lookup_prologue(idx, off, tables, p, q, _pad(r))
    plan_rows = E_.make_plan(tables, p, q, _pad(r), idx.numel(), idx, tab, None)
    inside = E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx, tab, packed)
    for plan in (plan_bags, plan_rows):
        assert torch.equal(E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx, tab, packed, plan), inside)
    assert torch.equal(E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx, tab, packed), inside)
    pooled = E_.bag_sum_pool(inside, off)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the capture's stream (its workspace)
        E_.bag_sum_pool(E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx, tab, packed), off)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        g_rows = E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx, tab, packed)
        g_out = E_.bag_sum_pool(g_rows, off)
    for k in range(3):
        g_rows.zero_(), g_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_rows, inside) and torch.equal(g_out, pooled), f"replay {k}"
    assert E_.tt_rows_bf16(tables, D, p, q, _pad(r), idx[:0], tab[:0], packed).shape == (0, D)


# ---------------------------------------------------------------------------------------------------------- bag_sum_pool
@pytest.mark.parametrize("D", [1, 3, 4, 64, 260])
def test_bag_sum_pool_is_the_sequential_float32_sum(D):
    import tt_embeddings as E_

    rs = np.random.RandomState(60 + D)
    lens = np.array([0, 1, 1000, 0, 0, 3, 17, 1, 0, 64, 5, 0], dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = (rs.standard_normal((int(off[-1]), D)) * 10.0 ** rs.randint(-3, 4, size=(int(off[-1]), 1))).astype(np.float32)
    got = E_.bag_sum_pool(t(rows), t(off)).cpu().numpy()
    want = R.pool_f32_sequential(rows, off)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert not got[[0, 3, 4, 8, 11]].any()
    if D % 4 == 0:  # rows that are not 16-byte aligned take the scalar path: the same sums
        buf = t(np.concatenate([np.zeros(1, np.float32), rows.reshape(-1)]))
        assert np.array_equal(E_.bag_sum_pool(buf[1:].view(-1, D), t(off)).cpu().numpy(), want)
    assert E_.bag_sum_pool(t(rows[:0]), t(np.zeros(1, np.int64))).shape == (0, D)  # nb == 0


# --------------------------------------------------------------------------------------------------------------- modules
def _source(kind, tables, q, r, p, mode, seed=71, **kw):
    import tt_embeddings_ops as ops

    E, D = int(np.prod(p)), int(np.prod(q))
    if kind == "batched":
        m = ops.TableBatchedTTEmbeddingBag(tables, E, D, list(r), list(p), list(q), weight_dist="uniform", device=dev(), mode=mode, **kw)
    elif kind == "bag":
        m = ops.TTEmbeddingBag(E, D, list(r), list(p), list(q), weight_dist="uniform", device=dev(), mode=mode, use_cache=False, **kw)
    else:
        m = ops.TTEmbedding(E, D, list(r), list(p), list(q), weight_dist="uniform", device=dev(), **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, G.make_cores(seed, m.num_tables, p, q, r, "signed")):
            dst.copy_(t(src))
    return m, E, D


def _ragged(rs, nb, E):
    lens = rs.randint(0, 6, size=nb)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return rs.randint(0, E, size=int(off[-1])).astype(np.int64), off


@pytest.mark.parametrize("kind,tables,mode", [("batched", 1, "sum"), ("batched", 3, "sum"), ("batched", 3, "mean"), ("bag", 1, "sum"),
                                              ("bag", 1, "mean"), ("embedding", 1, "sum")])
def test_from_module_serves_within_the_pooled_bound(kind, tables, mode):
    import ttx_infer

    q, r, p = [4, 4, 4], [32, 32], P_B
    m, E, D = _source(kind, tables, q, r, p, mode)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    inf = ttx_infer.TTInferenceBag.from_module(m)
    assert inf.route == "bf16" and not list(inf.parameters()) and len(list(inf.buffers())) == 3
    cores = [R.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores]
    rs = np.random.RandomState(72)
    if kind == "embedding":
        idx = rs.randint(0, E, size=(4, 9)).astype(np.int64)
        ti = t(idx)
        call = lambda: inf(ti)  # noqa: E731
        ref, bnd = R.rows64(*R.slices(cores, p, q, r, idx.reshape(-1), np.zeros(idx.size, np.int64)))
        shape = (4, 9, D)
    else:
        B = 9
        idx, off = _ragged(rs, tables * B, E)
        ti, to = t(idx), t(off)
        call = lambda: inf(ti, to)  # noqa: E731
        tab = np.repeat(np.arange(tables * B) // B, np.diff(off))
        ref, bnd = R.pool64(*R.rows64(*R.slices(cores, p, q, r, idx, tab)), off, mean=mode == "mean")
        shape = (B, D) if kind == "bag" else (tables, B, D)
    out = call()
    assert tuple(out.shape) == shape and out.dtype == torch.float32 and not out.requires_grad
    err = np.abs(out.cpu().numpy().astype(np.float64).reshape(ref.shape) - ref)
    ratio = float(np.max(err / np.maximum(bnd, 1e-300)))
    print(f"{kind} tables={tables} {mode}: worst err / pooled bound {ratio:.5f}")
    assert (err <= bnd).all(), ratio
    after = m.state_dict()
    assert list(before) == list(after) and all(torch.equal(before[k], after[k]) for k in before)
    # a captured forward replayed equals eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        g_out = call()
    for _ in range(2):
        g_out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_out, out)


@pytest.mark.parametrize("case", ["T2", "T4", "r128"])
def test_unsupported_sources_fall_back_to_fp32_on_the_rounded_cores(case):
    import tt_embeddings_ops as ops
    import ttx_infer

    if case == "r128":
        p, q, r = P_A, [4, 4, 4], [128, 128]
    else:
        p, q, r = G.test_shape(2 if case == "T2" else 4)
    tables, B = 2, 7
    E, D = int(np.prod(p)), int(np.prod(q))
    m = ops.TableBatchedTTEmbeddingBag(tables, E, D, list(r), list(p), list(q), weight_dist="uniform", device=dev(), mode="mean")
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, G.make_cores(81, tables, p, q, r, "signed")):
            dst.copy_(t(src))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    inf = ttx_infer.TTInferenceBag.from_module(m)
    assert inf.route == "fp32" and not list(inf.parameters())
    assert all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    idx, off = _ragged(np.random.RandomState(82), tables * B, E)
    out = inf(t(idx), t(off))
    assert not out.requires_grad and tuple(out.shape) == (tables, B, D)
    with torch.no_grad():
        for c in m.tt_cores:
            c.copy_(c.to(torch.bfloat16).float())
        ref = m(t(idx), t(off))
    assert torch.equal(out, ref)
