"""CPU tests (no GPU) of from_pretrained / truncate_ranks: TT-SVD of a dense table and TT rounding (fbtt-embedding_amd/ttx_svd.py),
the canonical-core accessors and `full_weight(table)` of the modules, and the modules built by `from_pretrained` on the oracle engine.

Every expected number comes from tests/svd_ref.py (float64 numpy: np.linalg.svd on the explicit unfoldings, an entry-by-entry
tt_full), never from the code under test.  Each property is checked on both routes of a truncation step: torch.linalg.svd on the
unfolding (what these small shapes take by default) and the Gram matrix of the unfolding's smaller side (forced by setting the
size switch `_SVD_DIRECT_MAX` to 0: what a real table takes).

The shapes are svd_ref.CASES.  A table of EXACT TT ranks exists only over all prod(p) rows: cutting a table of ranks R to E < prod(p)
rows and zero-padding it again is subtracting a corner block, which raises the ranks (up to 2 R).  So the exact-recovery, rank-selection
and rounding tests take the prod(p) rows of a table built from cores, and the padded rows (E < prod(p): 57 of 60, 23 of 24,
117 of 120) are covered where no exact rank is needed: truncation of full-rank tables and the modules.

Tolerances: 1e-5 relative to ||W||_F is the project's default relative tolerance (util.RTOL); the float32 rounding of the returned
cores moves the table by about 1e-7 ||W||_F (measured below, printed by every test before it asserts)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import svd_ref as R
from test_mixed_modes_cpu import Engine
from util import RTOL, assert_close

TRUNC = {"T3": [3, 2], "T2": [3], "T4": [2, 3, 2], "cap": [7, 4]}      # ranks below what full-rank tables of the shapes have
EXACT = {"T3": [4, 3], "T2": [5], "T4": [3, 4, 3], "cap": [3, 2]}      # the exact ranks of the rank-selection / rounding tables
E_TRUNC = {"T3": 57, "T2": 23, "T4": 117, "cap": 57}                   # E < prod(p): padded rows
NAMES = list(R.CASES)
ROUTES = ["svd", "gram"]


@pytest.fixture()
def svd(monkeypatch, request):
    import ttx_svd

    route = getattr(request, "param", "svd")
    if route == "gram":
        monkeypatch.setattr(ttx_svd, "_SVD_DIRECT_MAX", 0)
    return ttx_svd


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", Engine())
    return m


def geometry(name):
    c = R.CASES[name]
    return c["p"], c["q"]


def f64(cores):
    return [c.detach().double().numpy() for c in cores]


def t32(cores):
    return [torch.from_numpy(np.asarray(c, dtype=np.float32)) for c in cores]


@functools.lru_cache(maxsize=None)
def exact_table(name, ranks=None):
    """(float32 cores of exactly `ranks`, their table over all prod(p) rows rounded to float32)"""
    p, q = geometry(name)
    rk = list(ranks) if ranks is not None else R.CASES[name]["ranks"]
    cores = R.random_cores(np.random.RandomState(len(name) + 11 * len(rk) + sum(rk)), p, q, rk)
    return cores, R.tt_full(cores).astype(np.float32)


@functools.lru_cache(maxsize=None)
def full_rank_table(name):
    p, q = geometry(name)
    return np.random.RandomState(7 + len(name)).standard_normal((E_TRUNC[name], int(np.prod(q)))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def trunc_ref(name):
    p, q = geometry(name)
    return R.tt_svd(full_rank_table(name), p, q, TRUNC[name])


# ------------------------------------------------------------------------------------------------------------------- layout
@pytest.mark.parametrize("name", NAMES)
def test_module_layout_round_trip(svd, name):
    p, q = geometry(name)
    cores = t32(exact_table(name)[0])
    mats = svd.to_module_layout(cores)
    r = [1] + R.CASES[name]["ranks"] + [1]
    assert [tuple(m.shape) for m in mats] == [(p[k], r[k] * q[k] * r[k + 1]) for k in range(len(p))]
    back = svd.from_module_layout(mats, q, R.CASES[name]["ranks"])
    assert all(torch.equal(a, b) for a, b in zip(back, cores))
    assert all(torch.equal(a, b) for a, b in zip(svd.from_module_layout(mats, q, r), cores)), "ranks as the modules keep them"


@pytest.mark.parametrize("name", NAMES)
def test_table_cores_expand_to_full_weight(ops, svd, name):
    p, q = geometry(name)
    torch.manual_seed(2)
    m = ops.TTEmbeddingBag(int(np.prod(p)), int(np.prod(q)), EXACT[name], p, q, use_cache=False, weight_dist="uniform", device="cpu")
    assert_close(svd.tt_full(m.table_cores()).numpy(), m.full_weight().detach().numpy(), "float32")
    assert torch.equal(m.full_weight(0), m.full_weight().detach()[:m.num_embeddings])
    m = m.double()
    assert m.table_cores()[0].dtype == torch.float64
    assert torch.equal(svd.tt_full(m.table_cores()), m.full_weight().detach()), "float64: the same operations, bit for bit"
    cores = m.table_cores()
    cores[0].mul_(2.0)
    assert not torch.equal(svd.tt_full(m.table_cores()), svd.tt_full(cores)), "table_cores returns copies"
    m.load_table_cores(cores)
    assert torch.equal(svd.tt_full(m.table_cores()), svd.tt_full(cores))


@pytest.mark.parametrize("name", NAMES)
def test_restatement_expands_like_the_reference_shaped_expansion(ops, svd, name):
    p, q = geometry(name)
    cores = [c.astype(np.float64) for c in exact_table(name)[0]]
    stored = [torch.from_numpy(c.transpose(1, 0, 2, 3).reshape(1, c.shape[1], -1).copy()) for c in cores]
    ref = ops.tt_matrix_to_full(p, q, R.CASES[name]["ranks"], stored, [1, 0, 2, 3]).numpy()
    np.testing.assert_allclose(R.tt_full(cores), ref, rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(svd.tt_full([torch.from_numpy(c) for c in cores], 7).numpy(), ref[:7], rtol=1e-12, atol=1e-13)


# ----------------------------------------------------------------------------------------------------------- exact recovery
@pytest.mark.parametrize("svd", ROUTES, indirect=True)
@pytest.mark.parametrize("name", NAMES)
def test_exact_recovery(svd, name):
    p, q = geometry(name)
    ranks = R.CASES[name]["ranks"]
    _, W = exact_table(name)
    res = svd.tt_svd(torch.from_numpy(W), p, q, ranks)
    r = [1] + ranks + [1]
    assert res.ranks == ranks, "the requested ranks, exactly -- zero-padded where an unfolding admits fewer"
    assert [tuple(c.shape) for c in res.cores] == [(r[k], p[k], q[k], r[k + 1]) for k in range(len(p))]
    assert all(c.dtype == torch.float32 for c in res.cores)
    norm = float(np.linalg.norm(W.astype(np.float64)))
    err = R.error(W, f64(res.cores))
    print(f"{name}: relative error {err / norm:.3e}, bound / norm {res.bound / norm:.3e}")
    assert abs(res.norm - norm) <= 1e-12 * norm
    assert err <= RTOL * norm
    assert res.bound <= 1e-6 * norm
    if name == "cap":  # n = [20, 8, 6]: the unfoldings admit ranks 20 and 6 -- the surplus of the 32s is zero
        assert all(float(c.abs().max()) == 0.0 for c in (res.cores[0][..., 20:], res.cores[1][20:], res.cores[1][..., 6:], res.cores[2][6:]))


# --------------------------------------------------------------------------------------------------------------- truncation
@pytest.mark.parametrize("svd", ROUTES, indirect=True)
@pytest.mark.parametrize("name", NAMES)
def test_truncation_error_against_the_restatement(svd, name):
    p, q = geometry(name)
    W, ref = full_rank_table(name), trunc_ref(name)
    assert W.shape[0] < int(np.prod(p))
    res = svd.tt_svd(torch.from_numpy(W), p, q, TRUNC[name])
    err, err_ref = R.error(W, f64(res.cores)), R.error(W, ref["cores"])
    floor = max(R.unfolding_tails(W, p, q, TRUNC[name]))
    print(f"{name}: error {err:.6f} restatement {err_ref:.6f} bound {ref['bound']:.6f} Eckart-Young floor {floor:.6f} norm {ref['norm']:.4f}")
    assert res.ranks == TRUNC[name] == ref["ranks"]
    assert abs(err - err_ref) <= RTOL * ref["norm"]
    assert err <= ref["bound"] * (1 + RTOL)
    assert err >= floor * (1 - RTOL)
    np.testing.assert_allclose(res.eps_k, ref["eps_k"], rtol=1e-6)
    np.testing.assert_allclose([res.bound, res.norm], [ref["bound"], ref["norm"]], rtol=1e-6)


# ----------------------------------------------------------------------------------------------------------- rank selection
@functools.lru_cache(maxsize=None)
def gapped_table(name):
    """a table of exact ranks EXACT[name] plus Gaussian noise of 1e-3 of its norm, all prod(p) rows"""
    _, W0 = exact_table(name, tuple(EXACT[name]))
    noise = np.random.RandomState(5).standard_normal(W0.shape)
    return (W0 + noise * (1e-3 * np.linalg.norm(W0) / np.linalg.norm(noise))).astype(np.float32)


@pytest.mark.parametrize("svd", ROUTES, indirect=True)
@pytest.mark.parametrize("name", NAMES)
def test_rank_selection_by_relative_error(svd, name):
    p, q = geometry(name)
    W, eps = gapped_table(name), 1e-2
    ref = R.tt_svd(W, p, q, rel_error=eps)
    delta = eps * ref["norm"] / np.sqrt(len(p) - 1)
    for S, r in zip(ref["sigma"], ref["ranks"]):  # the restatement alone decides that the case is valid
        assert S[r - 1] >= 10 * S[r], "the threshold must fall into a 10x gap of the singular values"
        assert np.sqrt((S[r:] ** 2).sum()) * 3 <= delta <= np.sqrt((S[r - 1:] ** 2).sum()) / 3, "... well inside it"
    assert ref["ranks"] == EXACT[name]
    res = svd.tt_svd(torch.from_numpy(W), p, q, rel_error=eps)
    err = R.error(W, f64(res.cores))
    print(f"{name}: ranks {res.ranks}, error / norm {err / ref['norm']:.3e}, bound / norm {res.bound / ref['norm']:.3e}")
    assert res.ranks == ref["ranks"]
    assert err <= eps * ref["norm"] * (1 + RTOL)
    assert res.bound <= eps * ref["norm"]
    cap = max(1, max(EXACT[name]) - 1)
    capped = svd.tt_svd(torch.from_numpy(W), p, q, rel_error=eps, max_rank=cap)
    assert capped.ranks == [min(r, cap) for r in EXACT[name]]
    assert abs(R.error(W, f64(capped.cores)) - R.error(W, R.tt_svd(W, p, q, capped.ranks)["cores"])) <= RTOL * ref["norm"]
    mult = svd.tt_svd(torch.from_numpy(W), p, q, rel_error=eps, rank_multiple=4)
    assert mult.ranks == [-(-r // 4) * 4 for r in EXACT[name]]
    assert [c.shape[3] for c in mult.cores[:-1]] == mult.ranks
    assert np.linalg.norm(R.tt_full(f64(mult.cores)) - R.tt_full(f64(res.cores))) <= RTOL * ref["norm"], "the function unchanged"
    assert mult.eps_k == res.eps_k


# ----------------------------------------------------------------------------------------------------------------- rounding
@pytest.mark.parametrize("svd", ROUTES, indirect=True)
@pytest.mark.parametrize("name", NAMES)
def test_rounding(svd, name):
    p, q = geometry(name)
    cores, _ = exact_table(name, tuple(EXACT[name]))
    full = R.tt_full(cores)
    norm = float(np.linalg.norm(full))
    lower = [max(1, r - 1) for r in EXACT[name]]
    ref = R.tt_svd(full, p, q, lower)
    err_ref = R.error(full, ref["cores"])
    res = svd.tt_round(t32(cores), lower)
    err = R.error(full, f64(res.cores))
    print(f"{name}: {EXACT[name]} -> {lower}: error {err:.6f} restatement {err_ref:.6f} norm {norm:.4f}")
    assert res.ranks == lower and all(c.dtype == torch.float32 for c in res.cores)
    assert abs(err - err_ref) <= RTOL * norm
    assert abs(res.norm - norm) <= 1e-6 * norm
    np.testing.assert_allclose(res.eps_k, ref["eps_k"], rtol=1e-6)
    higher = [r + 2 for r in EXACT[name]]
    same = svd.tt_round(t32(cores), higher)
    assert same.ranks == higher and [c.shape[3] for c in same.cores[:-1]] == higher
    assert R.error(full, f64(same.cores)) <= RTOL * norm, "ranks at or above the cores': the table unchanged"
    assert same.bound <= 1e-6 * norm
    padded = svd.tt_round(t32(R.pad_ranks(cores, [r + 3 for r in EXACT[name]])), lower)
    assert abs(R.error(full, f64(padded.cores)) - err_ref) <= RTOL * norm, "zero-padded surplus ranks: the unpadded error"
    chosen = svd.tt_round(t32(R.pad_ranks(ref["cores"], higher)), rel_error=1e-3, rank_multiple=2)
    assert chosen.ranks == [-(-r // 2) * 2 for r in lower], "the surplus is found by its (zero) singular values"
    assert R.error(R.tt_full(ref["cores"]), f64(chosen.cores)) <= 1e-3 * norm


# ------------------------------------------------------------------------------------------------------------------ modules
def bags_over_all_rows(Es):
    """table-major (indices, offsets): B = max(E) bags, bag b of table k holds row b (empty past E_k)"""
    B = max(Es)
    idx = torch.cat([torch.arange(e) for e in Es])
    off, base = [], 0
    for e in Es:
        off.append(torch.clamp(torch.arange(B), max=e) + base)
        base += e
    return idx, torch.cat(off + [torch.tensor([base])]), B


def check_member(what, full_weight, W, name):
    """full_weight within the restatement's error of the input `W` (a full-rank table truncated to TRUNC[name])"""
    ref = trunc_ref(name)
    assert tuple(full_weight.shape) == W.shape
    err = float(np.linalg.norm(full_weight.double().numpy() - W.astype(np.float64)))
    err_ref = float(np.linalg.norm(R.tt_full(ref["cores"], W.shape[0]) - W))
    print(f"{what}: error {err:.6f} restatement {err_ref:.6f}")
    assert abs(err - err_ref) <= RTOL * ref["norm"], what


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kind", ["TTEmbeddingBag", "TTEmbedding"])
def test_one_table_modules_from_pretrained(ops, name, kind):
    p, q = geometry(name)
    W = full_rank_table(name)
    E, D = W.shape
    cls = getattr(ops, kind)
    kw = dict(device="cpu", optimizer=ops.OptimType.EXACT_ADAGRAD, use_cache=False)
    m = cls.from_pretrained(torch.from_numpy(W), TRUNC[name], p, q, **kw)
    assert type(m) is cls and m.num_embeddings == E and m.tt_ranks == [1] + TRUNC[name] + [1]
    check_member(f"{kind} {name}", m.full_weight(0), W, name)
    idx = torch.arange(E)
    if kind == "TTEmbedding":
        out, ref = m(idx), F.embedding(idx, m.full_weight(0))
    else:
        out, ref = m(idx, torch.arange(E + 1)), F.embedding_bag(idx, m.full_weight(0), torch.arange(E + 1), mode="sum", include_last_offset=True)
    assert_close(out.detach().numpy(), ref.numpy(), f"{kind} {name} forward")
    twin = cls(E, D, TRUNC[name], p, q, weight_dist="uniform", **kw)
    assert list(m.state_dict()) == list(twin.state_dict())
    assert all(float(s.abs().max()) == 0.0 for s in m.optimizer_state), "optimizer state starts at zero"
    (ranks, bound, norm), = m.compression
    ref = trunc_ref(name)
    assert ranks == TRUNC[name]
    np.testing.assert_allclose([bound, norm], [ref["bound"], ref["norm"]], rtol=1e-6)


def test_default_shapes_are_the_constructors(ops):
    W = torch.from_numpy(np.random.RandomState(1).standard_normal((57, 24)).astype(np.float32))
    m = ops.TTEmbeddingBag.from_pretrained(W, [2, 2], device="cpu", use_cache=False)
    twin = ops.TTEmbeddingBag(57, 24, [2, 2], device="cpu", use_cache=False)
    assert (m.tt_p_shapes, m.tt_q_shapes) == (twin.tt_p_shapes, twin.tt_q_shapes)
    m = ops.TTEmbeddingBag.from_pretrained(W, rel_error=0.5, device="cpu", use_cache=True, cache_size=5)
    assert m.tt_ndim == 3 and m.use_cache and m.warmup, "three cores as the constructors' default; a cache starts in warm-up"
    ranks, bound, norm = m.compression[0]
    assert m.tt_ranks == [1] + ranks + [1] and bound <= 0.5 * norm
    assert float((m.full_weight(0) - W).norm()) <= 0.5 * norm * (1 + RTOL)


def test_batched_module_from_pretrained(ops):
    name = "T3"
    p, q = geometry(name)
    W = full_rank_table(name)
    E, D = W.shape
    both = [W, (W[::-1] * 0.5).copy()]
    for emb in (torch.from_numpy(np.stack(both)), [torch.from_numpy(w) for w in both]):
        m = ops.TableBatchedTTEmbeddingBag.from_pretrained(emb, TRUNC[name], p, q, device="cpu")
        assert m.num_tables == 2 and m.tt_ranks == [1] + TRUNC[name] + [1]
        check_member("batched table 0", m.full_weight(0), W, name)
        ref1 = R.tt_svd(both[1], p, q, TRUNC[name])
        err1 = float(np.linalg.norm(m.full_weight(1).double().numpy() - both[1]))
        assert abs(err1 - np.linalg.norm(R.tt_full(ref1["cores"], E) - both[1])) <= RTOL * ref1["norm"]
    idx, off, B = bags_over_all_rows([E, E])
    out = m(idx, off)
    for k in range(2):
        assert_close(out[k].detach().numpy(), m.full_weight(k).numpy(), f"forward table {k}")
    twin = ops.TableBatchedTTEmbeddingBag(2, E, D, TRUNC[name], p, q, device="cpu", weight_dist="uniform")
    assert list(m.state_dict()) == list(twin.state_dict())
    assert [c[0] for c in m.compression] == [TRUNC[name]] * 2
    with pytest.raises(AssertionError):
        m.full_weight()  # (no argument, several tables: as before)
    # rel_error: every table at its own ranks, the module at the per-position maximum
    _, low = exact_table(name, (2, 2))
    _, high = exact_table(name, (4, 3))
    m = ops.TableBatchedTTEmbeddingBag.from_pretrained([torch.from_numpy(low), torch.from_numpy(high)], None, p, q, rel_error=1e-3,
                                                       device="cpu")
    assert [c[0] for c in m.compression] == [[2, 2], [4, 3]] and m.tt_ranks == [1, 4, 3, 1]
    for k, w in enumerate((low, high)):
        assert float(np.linalg.norm(m.full_weight(k).double().numpy() - w)) <= 1e-3 * np.linalg.norm(w)
    assert float(m.table_cores(0)[1][2:].abs().max()) == 0.0, "table 0 is zero-padded past its own ranks"


VAR_P = [[3, 4, 5], [2, 5, 4]]
VAR_E = [57, 37]


@functools.lru_cache(maxsize=None)
def var_tables():
    rs = np.random.RandomState(21)
    return [rs.standard_normal((e, 24)).astype(np.float32) for e in VAR_E]


def check_var_member(what, full_weight, k, ranks):
    W = var_tables()[k]
    ref = R.tt_svd(W, VAR_P[k], [2, 3, 4], ranks)
    err = float(np.linalg.norm(full_weight.double().numpy() - W))
    assert tuple(full_weight.shape) == W.shape
    assert abs(err - np.linalg.norm(R.tt_full(ref["cores"], W.shape[0]) - W)) <= RTOL * ref["norm"], what


def test_var_table_module_from_pretrained(ops):
    import ttx_mixed

    q, ranks = [2, 3, 4], [3, 2]
    tables = [torch.from_numpy(w) for w in var_tables()]
    m = ttx_mixed.VarTableTTEmbeddingBag.from_pretrained(tables, ranks, VAR_P, q, device="cpu")
    assert m.table_num_embeddings == VAR_E and m.tt_p_shapes == VAR_P
    for k in range(2):
        check_var_member(f"var table {k}", m.full_weight(k), k, ranks)
    idx, off, B = bags_over_all_rows(VAR_E)
    out = m(idx, off)
    for k, e in enumerate(VAR_E):
        assert_close(out[k, :e].detach().numpy(), m.full_weight(k).numpy(), f"forward table {k}")
        assert float(out[k, e:].detach().abs().sum()) == 0.0
    twin = ttx_mixed.VarTableTTEmbeddingBag(VAR_E, 24, ranks, VAR_P, q, device="cpu", weight_dist="uniform")
    assert list(m.state_dict()) == list(twin.state_dict())
    assert [c[0] for c in m.compression] == [ranks, ranks]
    with pytest.raises(NotImplementedError):
        m.full_weight()  # (no argument: as before)
    # smaller ranks go into the leading block, the rest is zero
    small = R.tt_svd(var_tables()[1], VAR_P[1], q, [2, 1])
    m.load_table_cores(t32(small["cores"]), 1)
    assert [tuple(c.shape) for c in m.table_cores(1)] == [(1, 2, 2, 3), (3, 5, 3, 2), (2, 4, 4, 1)]
    np.testing.assert_allclose(m.full_weight(1).numpy(), R.tt_full(small["cores"], VAR_E[1]), rtol=1e-5, atol=1e-5)
    assert float(m.table_cores(1)[1][2:].abs().max()) == 0.0 and float(m.table_cores(1)[1][..., 1:].abs().max()) == 0.0
    check_var_member("table 0 is untouched", m.full_weight(0), 0, ranks)
    with pytest.raises(ValueError):
        m.load_table_cores(t32(R.pad_ranks(small["cores"], [4, 2])), 1)  # (above the module's ranks)
    with pytest.raises(NotImplementedError, match="table_q"):
        ttx_mixed.VarTableTTEmbeddingBag(VAR_E, 24, ranks, VAR_P, [2, 3, 4], table_q=[[2, 3, 4], [2, 3, 4]], device="cpu").table_cores(0)


@pytest.mark.parametrize("fused", [False, True], ids=["grouped", "fused"])
def test_mixed_module_from_pretrained(ops, fused):
    import ttx_mixed

    q, ranks = [2, 3, 4], [3, 2]
    small = np.random.RandomState(3).standard_normal((7, 24)).astype(np.float32)
    tables = [torch.from_numpy(var_tables()[0]), torch.from_numpy(small), torch.from_numpy(var_tables()[1])]
    ps = [VAR_P[0], None, VAR_P[1]]
    m = ttx_mixed.MixedTTEmbeddingBag.from_pretrained(tables, ranks, ps, q, device="cpu", fused=fused, dense_below=10)
    assert m.dense_tables == [False, True, False] and m.num_embeddings == [57, 7, 37]
    check_var_member("mixed table 0", m.full_weight(0), 0, ranks)
    check_var_member("mixed table 2", m.full_weight(2), 1, ranks)
    assert torch.equal(m.full_weight(1), tables[1]), "a dense member: a copy of its rows"
    m.full_weight(1).zero_()
    assert torch.equal(m.full_weight(1), tables[1])
    assert m.compression[1] is None and [m.compression[k][0] for k in (0, 2)] == [ranks, ranks]
    twin = ttx_mixed.MixedTTEmbeddingBag([57, 7, 37], 24, ranks, ps, q, device="cpu", fused=fused, dense_below=10, weight_dist="uniform")
    assert list(m.state_dict()) == list(twin.state_dict())
    with pytest.raises(ValueError, match="dense member"):
        m.table_cores(1)
    # per-table ranks as in the constructor; no dense member: the forward runs on the CPU engine
    per_table = [[3, 2], [2, 2]]
    tt_only = [tables[0], tables[2]]
    m = ttx_mixed.MixedTTEmbeddingBag.from_pretrained(tt_only, per_table, VAR_P, q, device="cpu", fused=fused, include_last_offset=True)
    for k in range(2):
        check_var_member(f"mixed per-table ranks {k}", m.full_weight(k), k, per_table[k])
        assert m.compression[k][0] == per_table[k]
    outs = m([torch.arange(37), torch.arange(37)], [torch.arange(38), torch.arange(38)])
    for k in range(2):
        assert_close(outs[k].detach().numpy(), m.full_weight(k)[:37].numpy(), f"mixed forward table {k}")
    m = ttx_mixed.MixedTTEmbeddingBag.from_pretrained(tt_only, None, VAR_P, q, rel_error=0.9, max_rank=2, device="cpu", fused=fused)
    assert all(max(c[0]) <= 2 for c in m.compression)


def test_dense_module_from_pretrained():
    import ttx_dense

    tables = [torch.from_numpy(w) for w in var_tables()]
    m = ttx_dense.DenseTableBatchedEmbeddingBag.from_pretrained(tables, device="cpu", mode="mean")
    assert m.table_num_embeddings == VAR_E and m.mode == "mean"
    assert all(torch.equal(m.table_weight(k), w) for k, w in enumerate(tables))
    with pytest.raises(ValueError):
        ttx_dense.DenseTableBatchedEmbeddingBag.from_pretrained(torch.zeros(2, 3, 4), device="cpu")


@pytest.mark.parametrize("kind", ["TTEmbeddingBag", "TTEmbedding", "TableBatchedTTEmbeddingBag"])
def test_truncate_ranks(ops, kind):
    name = "T3"
    p, q = geometry(name)
    cores, W = exact_table(name)
    cls = getattr(ops, kind)
    emb = torch.from_numpy(W) if kind != "TableBatchedTTEmbeddingBag" else [torch.from_numpy(W), torch.from_numpy(W * 2)]
    kw = dict(device="cpu", optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=0.03, padding_idx=5)
    if kind != "TTEmbedding":
        kw.update(mode="mean", include_last_offset=False)
    if kind == "TTEmbeddingBag":
        kw.update(use_cache=True, cache_size=9, hashtbl_size=40)
    m = cls.from_pretrained(emb, [4, 3], p, q, **kw)
    low = m.truncate_ranks([2, 2])
    assert type(low) is cls and low is not m and m.tt_ranks == [1, 4, 3, 1]
    assert low.tt_ranks == [1, 2, 2, 1] and (low.tt_p_shapes, low.tt_q_shapes) == (m.tt_p_shapes, m.tt_q_shapes)
    assert (low.num_tables, low.num_embeddings, low.embedding_dim) == (m.num_tables, m.num_embeddings, m.embedding_dim)
    assert low._ctor_kwargs() == m._ctor_kwargs(), "the constructor arguments match apart from the ranks"
    assert low.learning_rate == 0.03 and low.padding_idx == 5 and low.optimizer == ops.OptimType.EXACT_ADAGRAD
    assert all(float(s.abs().max()) == 0.0 and s.shape == c.shape for s, c in zip(low.optimizer_state, low.tt_cores))
    full = R.tt_full(cores)
    ref = R.tt_svd(full, p, q, [2, 2])
    for k in range(m.num_tables):
        err = float(np.linalg.norm(low.full_weight(k).double().numpy() - (k + 1) * W))
        assert abs(err - (k + 1) * R.error(full, ref["cores"])) <= RTOL * (k + 1) * ref["norm"]
        assert low.compression[k][0] == [2, 2]
    chosen = m.truncate_ranks(rel_error=1e-3, rank_multiple=4)
    assert chosen.tt_ranks == [1, 4, 4, 1] and chosen.compression[0][0] == [4, 4]
    assert float(np.linalg.norm(chosen.full_weight(0).double().numpy() - W)) <= 1e-3 * ref["norm"]
    if kind == "TTEmbeddingBag":
        assert low.use_cache and low.warmup and tuple(low.cache_weight.shape) == (9, 24) and low.hashtbl.numel() == 40
        m.cache_populate()
        assert not m.warmup
        with pytest.raises(RuntimeError, match="live cache"):
            m.truncate_ranks([2, 2])
        with pytest.raises(RuntimeError, match="live cache"):
            m.load_table_cores(m.table_cores())


def test_truncate_ranks_is_refused_on_the_var_table_module(ops):
    import ttx_mixed

    m = ttx_mixed.VarTableTTEmbeddingBag(VAR_E, 24, [3, 2], VAR_P, [2, 3, 4], device="cpu", weight_dist="uniform")
    with pytest.raises(NotImplementedError):
        m.truncate_ranks([2, 2])


# ------------------------------------------------------------------------------------------------------------------- errors
def test_argument_errors(ops, svd, monkeypatch):
    p, q = geometry("T3")
    W = torch.from_numpy(full_rank_table("T3"))

    def no_arithmetic(*a, **kw):
        raise AssertionError("argument errors are raised before any arithmetic")

    for fn in ("svd", "eigh", "qr"):
        monkeypatch.setattr(torch.linalg, fn, no_arithmetic)
    bad = [
        dict(weight=W, p=p, q=[2, 3, 5], ranks=[2, 2]),                    # prod(q) != D
        dict(weight=W, p=[3, 4, 4], q=q, ranks=[2, 2]),                    # prod(p) < E
        dict(weight=W, p=p, q=q, ranks=[2]),                               # a number of ranks other than T - 1
        dict(weight=W, p=p, q=q, ranks=[2, 2, 2]),
        dict(weight=W, p=p, q=q, ranks=[2, 0]),                            # a non-positive rank
        dict(weight=W, p=p, q=q, ranks=[-1, 2]),
        dict(weight=W, p=p, q=q, ranks=[2, 2], rel_error=0.1),             # both
        dict(weight=W, p=p, q=q),                                          # neither
        dict(weight=W, p=p, q=q, rel_error=0.0),                           # rel_error outside (0, 1)
        dict(weight=W, p=p, q=q, rel_error=1.0),
        dict(weight=W, p=p, q=q, rel_error=-0.5),
        dict(weight=W.long(), p=p, q=q, ranks=[2, 2]),                     # a non-floating weight
        dict(weight=W[0], p=p, q=q, ranks=[2, 2]),                         # a non-2-D weight
        dict(weight=W[None], p=p, q=q, ranks=[2, 2]),
        dict(weight=W, p=p + [1, 1], q=q + [1, 1], ranks=[2, 2, 1, 1]),    # five cores
        dict(weight=W, p=p, q=q, rel_error=0.1, rank_multiple=0),
        dict(weight=W, p=p, q=q, rel_error=0.1, max_rank=0),
    ]
    for case in bad:
        kw = {k: case[k] for k in ("rel_error", "max_rank", "rank_multiple") if k in case}
        with pytest.raises(ValueError):
            svd.tt_svd(case["weight"], case["p"], case["q"], case.get("ranks"), **kw)
        if case["weight"] is W and len(case["p"]) == 3:
            with pytest.raises(ValueError):
                ops.TTEmbeddingBag.from_pretrained(W, case.get("ranks"), case["p"], case["q"], device="cpu", **kw)
    cores = t32(exact_table("T3")[0])
    for args, kw in (((cores, [2]), {}), ((cores, [2, 0]), {}), ((cores, [2, 2]), dict(rel_error=0.1)), ((cores,), {}),
                     ((cores,), dict(rel_error=2.0)), ((cores[:1], []), {}), (([cores[0], cores[2]], [4]), {})):
        with pytest.raises(ValueError):
            svd.tt_round(*args, **kw)
    with pytest.raises(ValueError):
        svd.tt_full([cores[1], cores[2]])
    m = ops.TTEmbeddingBag(60, 24, [4, 3], p, q, use_cache=False, device="cpu", weight_dist="uniform")
    with pytest.raises(ValueError):
        m.load_table_cores(cores[:2])
    with pytest.raises(ValueError):
        m.load_table_cores(t32(R.pad_ranks(exact_table("T3")[0], [5, 3])))
    with pytest.raises(ValueError):
        m.load_table_cores([c.transpose(1, 2).contiguous() for c in cores])
    with pytest.raises(IndexError):
        m.table_cores(1)
    with pytest.raises(ValueError):
        ops.TTEmbeddingBag.from_pretrained(torch.zeros(2, 60, 24), [4, 3], p, q, device="cpu")
    with pytest.raises(ValueError):
        ops.TableBatchedTTEmbeddingBag.from_pretrained(torch.zeros(60, 24), [4, 3], p, q, device="cpu")
    with pytest.raises(TypeError):
        ops.TTEmbeddingBag.from_pretrained(W, [2, 2], p, q, device="cpu", freeze=True)  # (there is no freeze keyword)
