"""The four-core route (csrc/ttx_tt.hip: t4_merge_dims, t4_merge_sorted_kernel / t4_merge_kernel, t4_grad23_mfma_kernel /
t4_grad23_kernel, t4_apply23_kernel) at every helper instantiation and on both sides of every batch-size switch, against the
float64 reference tests/tt_ref64.py.

The route's host code picks, per launch: the merge's form and positions per work-group, SEG (where a run's sum of d core_2 is
left and where the apply kernel looks for it), the gradient helper and its dynamic LDS.  tests/t4_ref.py mirrors those choices;
tests/test_t4_routes_cpu.py holds the mirror against the sources and the case table below against the mirror.  Here every launch
goes through the test library, whose host code reports what it chose (ttx_debug_t4_route), and every case asserts that report
against the mirror -- a threshold that moves without the table fails before any number is compared.

(a) the instantiation table (t4_ref.INSTANCES) at about 300 lookups, one and three tables;
(b) designed index sets (digit by digit, t4_ref.run_counts / core3_counts): core-2 runs of 1, SEG - 1, SEG, SEG + 1 and 5 SEG + 3
    lookups, runs that begin and end on a multiple of SEG, slices without a lookup in cores 2 and 3, a core-3 slice of one row and
    one of at least 8 G + 1, a total that is no multiple of 16;
(c) nnz = 2^k - 1 and 2^k for k = 14 .. 18 on the three smallest geometries (D = 16), the runs of (b) scaled to the SEG in force
    plus one slice that holds half of all lookups;
(d) the backward on the forward's plan (M reused) against the backward on a fresh plan (M recomputed): bit-identical;
(e) every case twice: bit-identical.

Per case: forward, dense gradients, fused SGD and fused Adagrad from tt_ref64.live_state against float64 (at 2^k - 1: forward and
dense); a dense gradient of zero and bit-identical weights and state on every slice without a lookup.  Tolerances: the default of
tests/util.py; wider only by tt_ref64.widen_factor on the fp32 oracle's own distance from float64 on the same case (capped at
WIDEN_CAP).  Every comparison prints its figures (pytest -s); profiles/t4_routes_tolerances.md has the widened ones."""
from math import gcd

import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import t4_ref as T4
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

ALL = ("fwd", "dense", "sgd", "adagrad")
HDR_T4_VALID = 20  # kHdrT4Valid (csrc/ttx_internal.h): 1 while the plan holds M of its lookups


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def _offsets(rs, n, bags):
    """ragged bags that sum to n, bag 3 empty"""
    cuts = np.sort(rs.randint(0, n + 1, bags - 2))
    return np.concatenate([[0], np.cumsum(np.insert(np.diff(np.concatenate([[0], cuts, [n]])), 3, 0))]).astype(np.int64)


def _finish(q, ranks, p, tables, B, idx, off, seed):
    r = G.pad_ranks(ranks, 4)
    D = int(np.prod(q))
    rowidx, tableidx = R.rowidx_from_offsets(off, tables)
    return dict(tables=tables, p=list(p), q=list(q), ranks=list(ranks), r=r, B=B, D=D, indices=idx.astype(np.int64), offsets=off,
                rowidx=rowidx, tableidx=tableidx, cores=G.make_cores(7 + seed, tables, p, q, r, "signed"),
                d_out=G.make_grad(13 + seed, tables, B, D))


def random_case(q, ranks, tables, per_table, seed):
    """(a): uniform rows of p = P4, `per_table` lookups per table over 8 ragged bags"""
    p, B = T4.P4, 8
    rs = np.random.RandomState(4000 + seed)
    idx = rs.randint(0, int(np.prod(p)), tables * per_table)
    off = np.concatenate([[0]] + [k * per_table + _offsets(rs, per_table, B)[1:] for k in range(tables)])
    return _finish(q, ranks, p, tables, B, idx, off, seed)


def _stride(n, near):
    s = max(1, near) | 1
    while gcd(s, n) != 1:
        s += 2
    return s


def designed_case(q, ranks, p, counts2, G3, B, seed):
    """(b), (c): one table; lookup j of n has the digits i_0 = j % p_0, i_1 = j / p_0 % p_1, i_2 by `counts2` (lookups per core-2
    slice), i_3 by t4_ref.core3_counts dealt with a stride coprime to n; the batch holds the lookups in another strided order"""
    n = int(sum(counts2))
    assert len(counts2) == p[2]
    j = np.arange(n, dtype=np.int64)
    i0, i1 = j % p[0], j // p[0] % p[1]
    i2 = np.repeat(np.arange(p[2], dtype=np.int64), counts2)
    i3 = np.repeat(np.arange(p[3], dtype=np.int64), T4.core3_counts(n, G3, p[3]))[j * _stride(n, n // 3) % n]
    idx = (((i0 * p[1] + i1) * p[2] + i2) * p[3] + i3)[j * _stride(n, n // 5) % n]
    c = _finish(q, ranks, p, 1, B, idx, _offsets(np.random.RandomState(seed), n, B), seed)
    c["counts2"], c["counts3"] = list(counts2), T4.core3_counts(n, G3, p[3])
    return c


# ---- the library on a case -------------------------------------------------------------------------------------------------------
def _grid(rec, q, ranks, nnz):
    if rec["merge"] == T4.SORTED:
        return (nnz + rec["merge_seg"] - 1) // rec["merge_seg"]
    return min(T4.T4_GRID_CAP, max(1, (nnz * ranks[1] * q[2] + 255) // 256))


def assert_route(E, c, what, backward):
    """the test library's report of its last four-core launch against the mirror; clears the report"""
    nnz = c["indices"].size
    rec, got = T4.route(c["q"], c["ranks"], nnz), E.debug_t4_route(clear=True)
    want = dict(merge_form=T4.FORM_ID[rec["merge"]], merge_seg=rec["merge_seg"], merge_grid=_grid(rec, c["q"], c["ranks"], nnz),
                seg=0, helper=0, lds_bytes=0, lds_opt_in=0, apply_seg=0, q3=0)
    if backward:
        want.update(seg=rec["SEG"], helper=T4.HELPER_ID[rec["helper"]], lds_bytes=rec["lds_bytes"], lds_opt_in=int(rec["lds_opt_in"]),
                    apply_seg=rec["SEG"], q3=rec["Q3"])
    assert got == want, f"{what}: the library chose {got}, the mirror says {want}"


def gpu(c, modes, state0=None, what=""):
    """the modes on the GPU through the test library, one plan -> dict(out, grads, sgd, ada_w, ada_s); every launch's route report
    is held against the mirror"""
    import tt_embeddings as E

    tables, p, q, r, B, D = c["tables"], c["p"], c["q"], c["r"], c["B"], c["D"]
    Lt = torch.zeros(4, dtype=torch.int64, device=dev())
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    res = {}
    with E.test_library():
        assert E.lib().ttx_debug_state() == 0 and E.lib().ttx_has_test_hooks() == 1
        colidx, rowidx, tableidx, ntt, _ = E.preprocess_indices_sync(t(c["indices"]), t(c["offsets"]), tables, True, e0, e1)
        nnz = colidx.numel()
        assert ntt == nnz == c["indices"].size
        plan = E.make_plan(tables, p, q, r, nnz, colidx, tableidx, rowidx)
        d_out = t(c["d_out"])
        args = (p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out)
        E.debug_t4_route(clear=True)
        if "fwd" in modes:
            cores = [t(x) for x in c["cores"]]
            res["out"] = E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, colidx, rowidx, tableidx, cores, plan=plan).cpu().numpy()
            assert_route(E, c, f"{what} forward", False)
        if "dense" in modes:
            cores = [t(x) for x in c["cores"]]
            res["grads"] = [g.cpu().numpy() for g in E.tt_dense_backward(1000, D, *args, cores, plan=plan)]
            assert_route(E, c, f"{what} dense", True)
            for k in range(4):
                assert np.array_equal(cores[k].cpu().numpy(), c["cores"][k]), f"{what}: the dense backward changed core {k}"
        if "sgd" in modes:
            cores = [t(x) for x in c["cores"]]
            E.tt_sgd_backward(1000, D, LR, *args, cores, plan=plan)
            res["sgd"] = [x.cpu().numpy() for x in cores]
            assert_route(E, c, f"{what} sgd", True)
        if "adagrad" in modes:
            cores, state = [t(x) for x in c["cores"]], [t(x) for x in state0]
            E.tt_adagrad_backward(1000, D, LR, EPS, *args, state, cores, plan=plan)
            res["ada_w"], res["ada_s"] = [x.cpu().numpy() for x in cores], [x.cpu().numpy() for x in state]
            assert_route(E, c, f"{what} adagrad", True)
    assert E.lib() is E._product
    return res


def bits_equal(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), \
        f"{what}: differs in {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} values"


class Oracle:
    """the fp32 oracle (oracle/ttx_oracle.c) on a case, run when a comparison first asks for it: the forward output, the dense
    gradients, and the cores one fp32 SGD step along them"""

    def __init__(self, c):
        self.c, self._out, self._g = c, None, None

    def _args(self):
        c = self.c
        return O.make_geom(c["tables"], c["p"], c["q"], c["r"]), c["B"], c["D"]

    def out(self):
        if self._out is None:
            g, B, D = self._args()
            self._out = O.tt_forward(g, B, D, self.c["indices"], self.c["rowidx"], self.c["tableidx"], self.c["cores"])
        return self._out

    def grad(self, k):
        if self._g is None:
            g, B, D = self._args()
            self._g = O.tt_backward(g, O.OPTIM_DENSE, B, D, 0, 0, self.c["indices"], self.c["rowidx"], self.c["tableidx"], self.c["d_out"],
                                    [x.copy() for x in self.c["cores"]])
        return self._g[k]

    def sgd(self, k):
        return self.c["cores"][k] - np.float32(LR) * self.grad(k)


def _close(what, got, ref, oracle):
    """got against float64 at the default tolerance; beyond it, at tt_ref64.widen_factor of the oracle's own distance from float64
    on the same case (oracle: a function that runs it -- a comparison inside the default bound passes at any factor and does not
    ask).  -> the factor"""
    u = R.default_units(got, ref)
    f, uo = (1.0, None) if u <= 1.0 else R.widen_factor(oracle(), ref)
    print(f"[t4-routes] {what}: kernel {u:.3f} default bounds from float64"
          + ("" if uo is None else f", oracle {uo:.3f} -> bound x{f:.2f}" + ("  WIDENED" if f > 1.0 else "")))
    assert_close(got, ref, f"{what} vs float64", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    return f


def check(c, what, modes=ALL, empty=()):
    """the whole comparison of one case (module docstring).  empty: cores that must have a slice without a lookup"""
    tables, p, q, r, B, D = c["tables"], c["p"], c["q"], c["r"], c["B"], c["D"]
    idx, rowidx, tableidx = c["indices"], c["rowidx"], c["tableidx"]
    rec = T4.route(q, c["ranks"], idx.size)
    assert rec is not None, f"{what}: the geometry does not take the four-core route"
    # ---- float64, and the fp32 oracle beside it ----
    ref = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, c["cores"], c["d_out"])
    mask = R.slice_mask(ref["touched"], c["cores"])
    for k in empty:
        assert not ref["touched"][k].all(), f"{what}: every slice of core {k} has a lookup"
    orc = Oracle(c)
    state0 = zeroed = None
    if "adagrad" in modes:
        state0, zeroed = R.live_state(ref["grads"], ref["touched"], 23 + idx.size)
    # ---- the library, twice ----
    on = gpu(c, modes, state0, what)
    again = gpu(c, modes, state0, what)
    for key in on:
        for k, (x, y) in enumerate(zip([on[key]] if key == "out" else on[key], [again[key]] if key == "out" else again[key])):
            bits_equal(x, y, f"{what} {key}[{k}]: run to run")
    _close(f"{what} out", on["out"], ref["out"], orc.out)
    fg = []
    for k in range(4):
        fg.append(_close(f"{what} grad{k}", on["grads"][k], ref["grads"][k], lambda: orc.grad(k)))
        assert mask[k].any() and not on["grads"][k][~mask[k]].any(), f"{what} grad{k}: a slice without a lookup has a gradient"
    if "sgd" in modes:
        e_sgd = R.sgd_step(c["cores"], ref["grads"], LR)
        for k in range(4):
            _close(f"{what} sgd core{k}", on["sgd"][k], e_sgd[k], lambda: orc.sgd(k))
            assert np.array_equal(on["sgd"][k][~mask[k]], c["cores"][k][~mask[k]]), f"{what} sgd core{k}: a slice without a lookup changed"
    if "adagrad" in modes:
        e_w, e_s = R.adagrad_step(c["cores"], state0, ref["grads"], ref["touched"], LR, EPS)
        for k in range(4):
            w, s = on["ada_w"][k], on["ada_s"][k]
            assert ref["touched"][k][zeroed[k]], "one TOUCHED slice per core starts from a zero state"
            assert np.array_equal(w[~mask[k]], c["cores"][k][~mask[k]]), f"{what} adagrad core{k}: weights of a slice without a lookup changed"
            assert np.array_equal(s[~mask[k]], state0[k][~mask[k]]), f"{what} adagrad core{k}: state of a slice without a lookup changed"
            print(f"[t4-routes] {what} adagrad core{k}: state {R.default_units(s, e_s[k]):.3f}, weights {R.default_units(w, e_w[k]):.3f} "
                  f"default bounds from float64 (gradient bound x{fg[k]:.2f})")
            R.assert_state_close(s, e_s[k], ref["grads"][k], f"{what} adagrad state{k} vs float64", scale=fg[k])
            assert_adagrad_close(w, e_w[k], ref["grads"][k], f"{what} adagrad core{k} vs float64", lr=LR, eps=EPS, state0=state0[k], scale=fg[k])


def reached(q, ranks, p):
    """the geometry leaves the generic kernels (ttx_debug_tiles reports no tiles) and merges, by the mirror"""
    import tt_embeddings as E

    assert T4.route(q, ranks, 1) is not None
    assert E.debug_tiles(1, p, q, G.pad_ranks(ranks, 4))["MC"] == 0, f"q = {q}, ranks {ranks} is not on the specialised kernels"


# ---- the tests ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T4.INSTANCES))
def test_instantiation(name):
    """(a), (e): one table of 301 lookups and three of 97 (neither total a multiple of 16: a partial last staging step)"""
    q, ranks, _, _ = T4.INSTANCES[name]
    reached(q, ranks, T4.P4)
    for tables, per_table in ((1, 301), (3, 97)):
        assert T4.seg(tables * per_table) == 16 and T4.merge_seg(tables * per_table) == 4
        check(random_case(q, ranks, tables, per_table, len(name) + 31 * tables), f"{name} {tables} x {per_table}")


@pytest.mark.parametrize("name", T4.STRUCT)
def test_run_structure(name):
    """(b) at SEG = 16: 134 lookups"""
    q, ranks, _, _ = T4.INSTANCES[name]
    p = T4.STRUCT_P
    reached(q, ranks, p)
    counts = T4.run_counts(16)
    n = sum(counts)
    rec = T4.route(q, ranks, n)
    G3 = rec["core3"][-1][1]   # (the pass with the most row groups)
    assert rec["SEG"] == 16 and n % 16 != 0 and counts[:4] == [16, 1, 15, 17] and counts[4] == 0 and counts[5] == 5 * 16 + 3
    c = designed_case(q, ranks, p, counts, G3, 8, 50 + len(name))
    c3 = c["counts3"]
    assert c3[0] == 1 and c3[1] == 0 and c3[2] >= 8 * G3 + 1
    check(c, f"{name} runs", empty=(2, 3))


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("k", T4.SWITCH_K)
@pytest.mark.parametrize("name", list(T4.SWITCH))
def test_batch_size_switch(name, k, side):
    """(c), (e): 2^k - 1 lookups (forward and dense gradients) and 2^k (every mode).  SEG doubles at k = 14, 16, 18, the sorted
    merge's positions per work-group grow at k = 15, 17 (tests/test_t4_routes_cpu.py holds the table to that); the library's
    report of both is asserted in every launch (assert_route)"""
    q, ranks = T4.SWITCH[name]
    p = T4.SWITCH_P
    reached(q, ranks, p)
    n, modes = ((1 << k) - 1, ("fwd", "dense")) if side == "below" else (1 << k, ALL)
    rec = T4.route(q, ranks, n)
    assert rec["SEG"] == {14: (16, 32), 15: (32, 32), 16: (32, 64), 17: (64, 64), 18: (64, 128)}[k][side == "at"]
    if rec["merge"] == T4.SORTED:
        assert rec["merge_seg"] == {14: (4, 4), 15: (4, 16), 16: (16, 16), 17: (16, 32), 18: (32, 32)}[k][side == "at"]
    counts = T4.run_counts(rec["SEG"], n)
    assert sum(counts) == n and counts[6] == n // 2
    check(designed_case(q, ranks, p, counts, rec["core3"][-1][1], 512, k), f"{name} n={n}", modes, empty=(2, 3))


def test_backward_on_the_forwards_m_is_the_backward_on_a_fresh_plan():
    """(d): after the forward the plan holds M and the mark (hdr[kHdrT4Valid]); the backward's merge launches leave at once.  On a
    freshly built plan they compute M again.  Same products in the same order: every gradient bit-identical."""
    import tt_embeddings as E

    q, ranks = T4.SWITCH["sorted_mfma4"]
    p, n = T4.SWITCH_P, T4.REUSE_NNZ
    rec = T4.route(q, ranks, n)
    assert rec["merge"] == T4.SORTED and rec["merge_seg"] == 16
    c = designed_case(q, ranks, p, T4.run_counts(rec["SEG"], n), rec["core3"][-1][1], 512, 77)
    r, B, D = c["r"], c["B"], c["D"]
    Lt = torch.zeros(4, dtype=torch.int64, device=dev())
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())

    def mark(plan):
        torch.cuda.synchronize()
        return int(plan.buf[:128].view(torch.int32)[HDR_T4_VALID])

    with E.test_library():
        colidx, rowidx, tableidx, _, _ = E.preprocess_indices_sync(t(c["indices"]), t(c["offsets"]), 1, True, e0, e1)
        cores, d_out = [t(x) for x in c["cores"]], t(c["d_out"])
        args = (p, q, r, Lt, n, colidx, rowidx, tableidx, d_out)
        plan = E.make_plan(1, p, q, r, n, colidx, tableidx, rowidx)
        assert mark(plan) == 0
        E.tt_forward(1000, 1, B, D, p, q, r, Lt, n, colidx, rowidx, tableidx, cores, plan=plan)
        assert mark(plan) == 1, "the forward's merge did not mark its M valid"
        reused = [g.cpu().numpy() for g in E.tt_dense_backward(1000, D, *args, cores, plan=plan)]
        assert mark(plan) == 1
        fresh_plan = E.make_plan(1, p, q, r, n, colidx, tableidx, rowidx)
        assert mark(fresh_plan) == 0
        fresh = [g.cpu().numpy() for g in E.tt_dense_backward(1000, D, *args, cores, plan=fresh_plan)]
        assert mark(fresh_plan) == 0, "only the forward's merge marks M"
        # ... and a fused step clears the mark: the next backward on that plan computes M from the updated cores
        E.tt_sgd_backward(1000, D, LR, *args, cores, plan=plan)
        assert mark(plan) == 0, "a fused write to cores 2 / 3 leaves the plan's M marked valid"
    for k in range(4):
        bits_equal(reused[k], fresh[k], f"grad{k}: M reused against M recomputed")
    ref = R.forward_backward(1, p, q, r, B, c["indices"], c["rowidx"], c["tableidx"], c["cores"], c["d_out"])
    orc = Oracle(c)
    for k in range(4):
        _close(f"reuse n={n} grad{k}", reused[k], ref["grads"][k], lambda: orc.grad(k))
