"""reduce_apply_small_kernel: the reduce + apply launch of a small batch -- eight half-waves per thin slice, a
float4 column of a pivot slice per thread, hot slices with segment / column work-groups of their own -- against the float64
restatement (tests/tt_ref64.py) at the suite's default tolerance (hot slices: widened by the fp32 oracle's own distance), against reduce_apply_kernel on the same launch (ttx_debug_skip bit 21, the test library) at that same tolerance (the
order of the fp32 additions differs: no bit equality), and against itself run twice (bit-identical).  Every case asserts the
kernel that ran (ttx_debug_reduce_route).

Shapes: p = [5, 6, 7], q = [4, 4, 4]; ranks [32, 32] (thin slices of 32 float4 lanes: whole half-waves), [16, 16] (16 lanes) and
[13, 12] (13 and 12 lanes, a pivot slice of 156); 1, 31, 64 and 700 lookups -- a single row; 12 thin slices (six work-groups, the
last slice of core 0 and the first of core 2 in one) of which some stay empty or hold fewer rows than half-waves; every slice
touched; slices of more than 64 rows, i.e. more than one round of loads.  p = [4, 6, 7]: an odd number of thin slices, the last
work-group holds one.  One skewed batch (700 lookups of ONE row: a hot slice in every core, which the segment and column
work-groups take), twelve hot pivot slices (more than the column split takes: their owners keep them), one case on each side of
the host's route bound (64 kSegThin = 16,384 lookups, every slice hot), and a geometry whose thin slices are no whole float4s
(q_0 = 2, r_1 = 13: 26 floats), which keeps reduce_apply_kernel."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import tt_ref64 as R
from util import ATOL_SCALE, LR, EPS, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

NO_SMALL = 1 << 21  # ttx_debug_skip: reduce_apply_kernel for every launch
FULL, SMALL = 1, 2  # ttx_debug_reduce_route (include/ttx_test_hooks.h)
ROUTE_BOUND = 64 * 256
P, Q, BAGS = [5, 6, 7], [4, 4, 4], 8
RANKS = {"r32": [32, 32], "r16": [16, 16], "r13x12": [13, 12]}
COUNTS = [1, 31, 64, 700]
MODES = ("dense", "sgd", "adagrad")


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


_CASES = {}


def case(ranks, n, q=None, skew=False, hot=False, p=None):
    """n lookups over 8 ragged bags of one table (uniform rows, or all of them row 77), the cores, the bag gradients and the float64
    reference -- made once per shape and left unchanged"""
    q, p = q or Q, p or P
    key = (tuple(ranks), n, tuple(q), skew, tuple(p))
    if key not in _CASES:
        rs = np.random.RandomState(9000 + n + 7 * ranks[0] + q[0])
        E_ = int(np.prod(p))
        idx = np.full(n, 77, dtype=np.int64) if skew else rs.randint(0, E_, n).astype(np.int64)
        cuts = np.sort(rs.randint(0, n + 1, BAGS - 1))
        off = np.concatenate([[0], cuts, [n]]).astype(np.int64)
        r = [1] + list(ranks) + [1]
        D = int(np.prod(q))
        c = dict(p=p, q=q, r=r, D=D, indices=idx, offsets=off, cores=G.make_cores(31 + n, 1, p, q, r, "signed"),
                 d_out=G.make_grad(37 + n, 1, BAGS, D))
        rowidx, tableidx = R.rowidx_from_offsets(off, 1)
        c["ref"] = R.forward_backward(1, p, q, r, BAGS, idx, rowidx, tableidx, c["cores"], c["d_out"])
        c["scale"] = [1.0, 1.0, 1.0]
        if hot:  # thousands of fp32 rows in one sum: the bound widens by the fp32 oracle's own distance from float64 (R.widen_factor)
            o = O.tt_backward(O.make_geom(1, p, q, r), O.OPTIM_DENSE, BAGS, D, 0, 0, idx, rowidx, tableidx, c["d_out"],
                              [x.copy() for x in c["cores"]])
            c["scale"] = [R.widen_factor(o[k], c["ref"]["grads"][k])[0] for k in range(3)]
            print(f"[reduce-small] n={n} skew={skew}: bounds widened by {c['scale']}")
        _CASES[key] = c
    return _CASES[key]


def run(c, mode, knob=0):
    """one backward through the test library -> (the arrays the mode produces, the reduce + apply kernel that ran)"""
    import tt_embeddings as E

    p, q, r, D = c["p"], c["q"], c["r"], c["D"]
    idx, off = t(c["indices"]), t(c["offsets"])
    Lt = torch.zeros(len(p), dtype=torch.int64, device=dev())
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    if knob:
        E.debug_skip(knob)
    try:
        with E.test_library():
            colidx, rowidx, tableidx, ntt, _ = E.preprocess_indices_sync(idx, off, 1, True, e0, e1)
            nnz = idx.numel()
            plan = E.make_plan(1, p, q, r, nnz, colidx, tableidx, rowidx)
            cores = [t(x) for x in c["cores"]]
            d_out = t(c["d_out"])
            res = {}
            if mode == "dense":
                grads = E.tt_dense_backward(1000, D, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, cores, plan=plan)
                res["grads"] = [g.cpu().numpy() for g in grads]
            elif mode == "sgd":
                E.tt_sgd_backward(1000, D, LR, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, cores, plan=plan)
            else:
                state = [torch.zeros_like(x) for x in cores]
                E.tt_adagrad_backward(1000, D, LR, EPS, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, state, cores, plan=plan)
                res["state"] = [s.cpu().numpy() for s in state]
            res["cores"] = [x.cpu().numpy() for x in cores]
            torch.cuda.synchronize()
            route = E.debug_reduce_route()
        return res, route
    finally:
        if knob:
            E.debug_skip(0)


def same(a, b, what):
    for key in a:
        for k, (x, y) in enumerate(zip(a[key], b[key])):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), \
                f"{what}: {key}[{k}] differs in {int((x.view(np.uint32) != y.view(np.uint32)).sum())} of {x.size} values"


def close(got, want, c, mode, what):
    """`got` against `want` (the float64 expectation, or the other kernel's arrays) at the default tolerance of the mode"""
    g64 = c["ref"]["grads"]
    for k in range(3):
        f = c["scale"][k]  # (1 but for the hot cases)
        if mode == "dense":
            assert_close(got["grads"][k], want["grads"][k], f"{what} grad{k}", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
        elif mode == "sgd":
            assert_close(got["cores"][k], want["cores"][k], f"{what} sgd core{k}", rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
        else:
            R.assert_state_close(got["state"][k], want["state"][k], g64[k], f"{what} adagrad state{k}", scale=f)
            assert_adagrad_close(got["cores"][k], want["cores"][k], g64[k], f"{what} adagrad core{k}", scale=f)


def expected(c, mode):
    ref = c["ref"]
    if mode == "dense":
        return {"grads": ref["grads"]}
    if mode == "sgd":
        return {"cores": R.sgd_step(c["cores"], ref["grads"], LR)}
    w, s = R.adagrad_step(c["cores"], [np.zeros_like(x) for x in c["cores"]], ref["grads"], ref["touched"], LR, EPS)
    return {"cores": w, "state": s}


def check(c, what, modes=MODES):
    for mode in modes:
        new, route = run(c, mode)
        assert route == SMALL, f"{what} {mode}: reduce_apply_small_kernel did not take the launch (route {route})"
        again, _ = run(c, mode)
        old, route_old = run(c, mode, NO_SMALL)
        assert route_old == FULL, f"{what} {mode}: the knob did not force reduce_apply_kernel (route {route_old})"
        same(new, again, f"{what} {mode}: run to run")
        close(new, expected(c, mode), c, mode, f"{what} vs float64:")
        close(new, old, c, mode, f"{what} vs reduce_apply_kernel:")
        if mode != "dense":  # (slices without a lookup keep their weights and their state, bit for bit)
            for k, m in enumerate(R.slice_mask(c["ref"]["touched"], c["cores"])):
                assert np.array_equal(new["cores"][k][~m], c["cores"][k][~m]), f"{what} {mode}: untouched slices of core {k} moved"


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("ranks", list(RANKS))
def test_small_launch(ranks, n):
    check(case(RANKS[ranks], n), f"{ranks} n={n}")


def test_odd_number_of_thin_slices():
    check(case(RANKS["r32"], 64, p=[4, 6, 7]), "p467 r32 n=64")


def test_hot_slices_of_a_single_row_batch():
    """700 lookups of one row: 700 partial rows in one slice of each thin core (hot: more than 2 kSegThin = 512: three segment
    work-groups and the last arriver's fold) and 44 chunk partials in one pivot slice (hot: more than 16: the column work-groups)"""
    check(case(RANKS["r32"], 700, skew=True, hot=True), "r32 skewed n=700")


def test_route_bound():
    """the largest launch the small kernel takes -- all twelve thin slices hot (64 segment work-groups per core, up to two hot
    slices in one of them) and all six pivot slices (every column work-group walks six) -- through every comparison of check()
    with the fused SGD update and the dense gradient; and the smallest launch it leaves to reduce_apply_kernel"""
    c = case(RANKS["r32"], ROUTE_BOUND, hot=True)
    check(c, f"r32 n={ROUTE_BOUND}", modes=("sgd", "dense"))
    c = case(RANKS["r32"], ROUTE_BOUND + 1, hot=True)
    new, route = run(c, "sgd")
    assert route == FULL, route
    close(new, expected(c, "sgd"), c, "sgd", f"r32 n={ROUTE_BOUND + 1} vs float64:")


def test_many_hot_pivot_slices_stay_with_their_owners():
    """p_1 = 12 at 8,192 lookups: twelve hot pivot slices of about 43 chunk partials, more than the eight the column split takes --
    their owners keep them (a thread per column, block sums), as reduce_apply_kernel's do"""
    check(case(RANKS["r32"], 8192, hot=True, p=[5, 12, 7]), "p5-12-7 r32 n=8192", modes=("adagrad", "dense"))


def test_thin_slices_that_are_no_whole_float4s_keep_the_full_kernel():
    c = case([13, 12], 64, q=[2, 4, 4])
    assert (c["r"][0] * c["q"][0] * c["r"][1]) % 4 != 0
    new, route = run(c, "sgd")
    assert route == FULL, route
    close(new, expected(c, "sgd"), c, "sgd", "q244 r13x12 n=64 vs float64:")
