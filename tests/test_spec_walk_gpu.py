"""The sub-chunk walk of every shape-specialised kernel that has one (csrc/ttx_tt_spec.inc: spec_fwd_kernel / spec_bwd_kernel
<MULTI> and <MULTI, PAD>), template by template, against the float64 reference tests/tt_ref64.py.

From 131,072 lookups per launch a template with Shape3::SUB is planned with chunks of four sub-chunks of Shape3::MC lookups: the
work-group walks them with the next sub-chunk's records and operands in flight and carries d core_1 in registers across the walk.
ttx_set_chunk(64) (test library) asks for that variant at any batch size, so a few hundred lookups reach it.  The case table is
tests/spec_ref.py's (held against the sources and against the template choice by tests/test_spec_walk_cpu.py): the eight templates
exact and padded, four cores merged onto each, and -- on S_32_8_32_8, the one template whose walk re-stages its core-1 block in every
column pass of every sub-chunk (MULTI && !B1ONCE), and on S2_16_4_16_4 -- per_sample_weights, a device-side live count, three tables
and a launch that mixes full and partial chunks of all core-1 slices.

Cases are built as tests/test_partial_stores_gpu.py builds them: all lookups of a table in ONE core-1 slice, so the count alone
decides the chunks (spec_ref.walk_counts), over 8 bags per table, one empty, the others ragged.

Per case, with the knob on: the plan's lookups per chunk are 4 Shape3::MC (Shape3::MC without the knob), the geometry runs on the
specialised kernels (ttx_debug_tiles reports no generic tiles; a padded one leaves them under ttx_debug_skip bit 15, exact shapes
only -- so the PAD variant is what ran); forward, dense gradients, fused SGD and fused Adagrad from tt_ref64.live_state against
float64; untouched slices bit-identical; two runs bit-identical.  (The live-count case runs the backward only: tt_forward takes no
device-side count.)

Knob on against knob off (the single-sub-chunk kernels on the same inputs).  Found in the code: a lookup's output row, its d core_0
partial and its d core_2 partial are computed by the same statements in both variants (spec_gemm_x0 and the tails; the 16-byte
stores of the exact single-sub-chunk kernels swap the MFMA operands -- the same products summed in the same order, as
tests/test_partial_stores_gpu.py holds bit for bit), and pooling and reduce_apply sum rows and per-lookup partials in an order that
does not depend on the chunk length.  So the forward output, d core_0 and d core_2 (four cores: d core_3 as well, from the same
per-lookup d M) are asserted BIT-IDENTICAL.  d core_1 is not: the walk adds the sub-chunks' products in registers (acc2p) and stores
one partial per chunk where the single-sub-chunk kernels store one per sub-chunk for reduce_apply to add -- another association.
It meets the float64 bound in both variants.

Tolerances: the default of tests/util.py; wider only by tt_ref64.widen_factor on the fp32 oracle's own distance from float64 on
the same case (capped).  Every comparison prints its figures (pytest -s); profiles/spec_walk_tolerances.md has the widened ones."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import spec_ref as SR
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

EXACT_ONLY = 1 << 15  # ttx_debug_skip: exact-shape templates only
BAGS = 8


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _bags(rs, n):
    """8 bag lengths that sum to n: bag 3 empty, the others ragged (zeros allowed)"""
    cuts = np.sort(rs.randint(0, n + 1, BAGS - 2))
    return np.insert(np.diff(np.concatenate([[0], cuts, [n]])), 3, 0)


def make_case(q, ranks, counts, tables=1, seed=0):
    """counts: lookups per table, all of table k in core-1 slice 2 + k -- or {core-1 slice: lookups} (one table, shuffled).  The
    other digits are uniform.  -> the case (p by the number of cores)"""
    T = len(q)
    p = SR.P3 if T == 3 else SR.P4
    by_slice = isinstance(counts, dict)
    total = sum(counts.values()) if by_slice else int(counts)
    rs = np.random.RandomState(1000 * seed + total + 7 * T)
    idx, lengths = [], []
    for k in range(tables):
        n = total
        i1 = np.full(n, 2 + k, dtype=np.int64)
        if by_slice:
            i1 = np.concatenate([np.full(c, s, dtype=np.int64) for s, c in counts.items()])
            rs.shuffle(i1)
        v = rs.randint(0, p[0], n) * p[1] + i1
        for c in range(2, T):
            v = v * p[c] + rs.randint(0, p[c], n)
        idx.append(v)
        lengths.append(_bags(rs, n))
    idx = np.concatenate(idx).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.int64)
    r = G.pad_ranks(ranks, T)
    D = int(np.prod(q))
    rowidx, tableidx = R.rowidx_from_offsets(off, tables)
    return dict(tables=tables, T=T, p=p, q=list(q), r=r, B=BAGS, D=D, indices=idx, offsets=off, rowidx=rowidx, tableidx=tableidx,
                cores=G.make_cores(7 + total, tables, p, q, r, "signed"), d_out=G.make_grad(13 + total, tables, BAGS, D))


def make_weights(seed, n):
    """[-0.5, 1.5), a tenth exactly 0"""
    rs = np.random.RandomState(seed)
    w = (rs.rand(n) * 2.0 - 0.5).astype(np.float32)
    w[rs.permutation(n)[: max(1, n // 10)]] = 0.0
    return w


# ---- the library on a case -------------------------------------------------------------------------------------------------------
def _mc_of(plan):
    torch.cuda.synchronize()
    return int(plan.buf[:8].view(torch.int32)[1])


def gpu(c, chunk, psw=None, live=None, state0=None, modes=("fwd", "dense", "sgd", "adagrad")):
    """every mode on the GPU, one plan -> dict(mc, out, grads, sgd, ada_w, ada_s).  chunk: ttx_set_chunk (64: the walk; 0: off)"""
    import tt_embeddings as E

    tables, p, q, r, B, D, T = c["tables"], c["p"], c["q"], c["r"], c["B"], c["D"], c["T"]
    Lt = torch.zeros(T, dtype=torch.int64, device=dev())
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    if chunk:
        E.set_chunk(chunk)
    try:
        assert (E.lib().ttx_debug_state() != 0) == bool(chunk)
        colidx, rowidx, tableidx, ntt, _ = E.preprocess_indices_sync(t(c["indices"]), t(c["offsets"]), tables, True, e0, e1)
        nnz = colidx.numel()
        assert ntt == nnz
        n_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev())
        plan = E.make_plan(tables, p, q, r, nnz, colidx, tableidx, rowidx, n_dev=n_dev)
        res = {"mc": _mc_of(plan)}
        w = None if psw is None else t(psw)
        d_out = t(c["d_out"])
        args = (p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out)
        if "fwd" in modes:
            cores = [t(x) for x in c["cores"]]
            res["out"] = E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, colidx, rowidx, tableidx, cores, plan=plan,
                                      per_sample_weights=w).cpu().numpy()
        if "dense" in modes:
            cores = [t(x) for x in c["cores"]]
            grads = E.tt_dense_backward(1000, D, *args, cores, plan=plan, per_sample_weights=w)
            res["grads"] = [g.cpu().numpy() for g in grads]
            for k in range(T):
                assert np.array_equal(cores[k].cpu().numpy(), c["cores"][k]), f"the dense backward changed core {k}"
        if "sgd" in modes:
            cores = [t(x) for x in c["cores"]]
            E.tt_sgd_backward(1000, D, LR, *args, cores, plan=plan, per_sample_weights=w)
            res["sgd"] = [x.cpu().numpy() for x in cores]
        if "adagrad" in modes:
            cores, state = [t(x) for x in c["cores"]], [t(x) for x in state0]
            E.tt_adagrad_backward(1000, D, LR, EPS, *args, state, cores, plan=plan, per_sample_weights=w)
            res["ada_w"], res["ada_s"] = [x.cpu().numpy() for x in cores], [x.cpu().numpy() for x in state]
        return res
    finally:
        if chunk:
            E.set_chunk(0)


def bits_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
        f"{what}: differs in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} values"


def _close(what, got, ref, oracle):
    """got against float64 at the default tolerance, or at tt_ref64.widen_factor of the oracle's own distance; -> the factor"""
    f, u = R.widen_factor(oracle, ref)
    print(f"[spec-walk] {what}: kernel {R.default_units(got, ref):.3f}, oracle {u:.3f} default bounds from float64 -> bound x{f:.2f}"
          + ("  WIDENED" if f > 1.0 else ""))
    assert_close(got, ref, f"{what} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    return f


def check(c, what, M, psw=None, live=None):
    """the whole comparison of one case (module docstring); M = Shape3::MC of its template"""
    tables, p, q, r, B, D, T = c["tables"], c["p"], c["q"], c["r"], c["B"], c["D"], c["T"]
    idx, rowidx, tableidx = c["indices"], c["rowidx"], c["tableidx"]
    n = idx.size if live is None else live
    modes = ("fwd", "dense", "sgd", "adagrad") if live is None else ("dense", "sgd", "adagrad")
    wl = None if psw is None else psw[:n]
    # ---- float64, and the fp32 oracle beside it ----
    ref = R.forward_backward(tables, p, q, r, B, idx[:n], rowidx[:n], tableidx[:n], c["cores"], c["d_out"], per_sample_weights=wl)
    mask = R.slice_mask(ref["touched"], c["cores"])
    if psw is None:
        g = O.make_geom(tables, p, q, r)
        o_out = O.tt_forward(g, B, D, idx[:n], rowidx[:n], tableidx[:n], c["cores"])
        o_g = O.tt_backward(g, O.OPTIM_DENSE, B, D, 0, 0, idx[:n], rowidx[:n], tableidx[:n], c["d_out"], [x.copy() for x in c["cores"]])
        o_w = [x.copy() for x in c["cores"]]
        O.tt_backward(g, O.OPTIM_SGD, B, D, LR, 0, idx[:n], rowidx[:n], tableidx[:n], c["d_out"], o_w)
    else:
        o_out, _, o_g, o_w = R.oracle_on_restatement(tables, p, q, r, B, idx[:n], rowidx[:n], tableidx[:n], wl, c["cores"], c["d_out"], LR)
    state0, zeroed = R.live_state(ref["grads"], ref["touched"], 23 + idx.size)
    e_sgd = R.sgd_step(c["cores"], ref["grads"], LR)
    e_w, e_s = R.adagrad_step(c["cores"], state0, ref["grads"], ref["touched"], LR, EPS)

    # ---- the walk, twice; the single-sub-chunk kernels once ----
    on = gpu(c, 64, psw, live, state0, modes)
    again = gpu(c, 64, psw, live, state0, modes)
    off = gpu(c, 0, psw, live, state0, tuple(m for m in modes if m in ("fwd", "dense")))
    assert on["mc"] == SR.SUBCHUNKS * M and off["mc"] == M, f"{what}: {on['mc']} / {off['mc']} lookups per chunk, Shape3::MC = {M}"
    for key in on:
        if key != "mc":
            for k, (x, y) in enumerate(zip([on[key]] if key == "out" else on[key], [again[key]] if key == "out" else again[key])):
                bits_equal(x, y, f"{what} {key}[{k}]: run to run")

    if "fwd" in modes:
        _close(f"{what} out", on["out"], ref["out"], o_out)
        _close(f"{what} out, knob off", off["out"], ref["out"], o_out)
        bits_equal(on["out"], off["out"], f"{what} out: the walk against the single-sub-chunk kernel")
    fg = []
    for k in range(T):
        fg.append(_close(f"{what} grad{k}", on["grads"][k], ref["grads"][k], o_g[k]))
        _close(f"{what} grad{k}, knob off", off["grads"][k], ref["grads"][k], o_g[k])
        if k != 1:
            bits_equal(on["grads"][k], off["grads"][k], f"{what} grad{k}: the walk against the single-sub-chunk kernel")
        assert mask[k].any() and not on["grads"][k][~mask[k]].any(), f"{what} grad{k}: an untouched slice has a gradient"
        _close(f"{what} sgd core{k}", on["sgd"][k], e_sgd[k], o_w[k])
        assert np.array_equal(on["sgd"][k][~mask[k]], c["cores"][k][~mask[k]]), f"{what} sgd core{k}: an untouched slice changed"
        w, s = on["ada_w"][k], on["ada_s"][k]
        assert ref["touched"][k][zeroed[k]], "one TOUCHED slice per core starts from a zero state"
        assert np.array_equal(w[~mask[k]], c["cores"][k][~mask[k]]), f"{what} adagrad core{k}: an untouched slice's weights changed"
        assert np.array_equal(s[~mask[k]], state0[k][~mask[k]]), f"{what} adagrad core{k}: an untouched slice's state changed"
        print(f"[spec-walk] {what} adagrad core{k}: state {R.default_units(s, e_s[k]):.3f}, weights {R.default_units(w, e_w[k]):.3f} "
              f"default bounds from float64 (gradient bound x{fg[k]:.2f})")
        R.assert_state_close(s, e_s[k], ref["grads"][k], f"{what} adagrad state{k} vs float64", scale=fg[k])
        assert_adagrad_close(w, e_w[k], ref["grads"][k], f"{what} adagrad core{k} vs float64", lr=LR, eps=EPS, state0=state0[k], scale=fg[k])


def reached(q, ranks, name, padded):
    """the geometry runs on the specialised kernels -- and, padded, only through the PAD variants; -> Shape3::MC"""
    import tt_embeddings as E

    T = len(q)
    p, r = (SR.P3 if T == 3 else SR.P4), G.pad_ranks(ranks, T)
    assert SR.match_any(q, ranks) == (name, padded)
    assert E.debug_tiles(1, p, q, r)["MC"] == 0, f"{name}: q = {q}, ranks {ranks} is not on the specialised kernels"
    if padded:
        E.debug_skip(EXACT_ONLY)
        try:
            assert E.debug_tiles(1, p, q, r)["MC"] != 0, f"{name}: q = {q}, ranks {ranks} stays on a template with exact shapes only"
        finally:
            E.debug_skip(0)
    assert E.hooks_lib().ttx_debug_state() == 0
    E._knobs_changed()
    return SR.SHAPES[name].MC


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["exact", "padded"])
@pytest.mark.parametrize("name", SR.SUB_TEMPLATES)
def test_walk_at_the_counts_that_decide_the_chunks(name, form):
    q, ranks = (SR.EXACT if form == "exact" else SR.PADDED)[name]
    M = reached(q, ranks, name, form == "padded")
    for n in SR.walk_counts(name):
        check(make_case(q, ranks, n), f"{name} {form} n={n}", M)


@pytest.mark.parametrize("name", SR.SUB_TEMPLATES)
def test_walk_under_four_cores(name):
    """the last two cores contracted per lookup (t4_merge_dims), then the three-core template's walk: all four cores against float64"""
    q, ranks = SR.FOUR_CORES[name]
    M = reached(q, ranks, name, False)
    for n in (3 * M - 1, 4 * M + 1):
        check(make_case(q, ranks, n), f"{name} four cores n={n}", M)


@pytest.mark.parametrize("kind", SR.EXTRA_KINDS)
@pytest.mark.parametrize("name", SR.EXTRA_TEMPLATES)
def test_walk_extra_cases(name, kind):
    q, ranks = SR.EXACT[name]
    s = SR.SHAPES[name]
    M = reached(q, ranks, name, False)
    if kind == "weights":
        n = 3 * M - 1
        check(make_case(q, ranks, n), f"{name} weights n={n}", M, psw=make_weights(5, n))
    elif kind == "live":
        check(make_case(q, ranks, 4 * M + 1), f"{name} {2 * M + 9} of {4 * M + 1} live", M, live=2 * M + 9)
    elif kind == "three_tables":
        check(make_case(q, ranks, 2 * M + 1, tables=3), f"{name} three tables", M)
    else:
        counts = {0: 1, 1: M - 1, 2: 2 * M + 1, 3: 5 * M, 4: s.LPG + 1, 5: 3 * M}
        assert len(counts) == SR.P3[1]
        check(make_case(q, ranks, counts), f"{name} all slices", M)
