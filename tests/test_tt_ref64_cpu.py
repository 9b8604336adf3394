"""CPU tests of the float64 TT reference (tests/tt_ref64.py) and of the apply-site classifier beside it:
  * the reference against the golden vectors made by the reference project's own Python (outputs, gradients, and the SGD / Adagrad
    expectations tests/util.py derives from them);
  * the fp32 oracle (oracle/ttx_oracle.c) against the reference in all four modes, Adagrad from a live state: the two CPU
    restatements pinned to each other;
  * the classifier's mirrored thresholds against the library's sources, and the classifier on hand-made batches;
  * per_sample_weights in the reference: `None` bit-identical to the reference before it had the argument, the weighted results
    against torch's F.embedding_bag and autograd in float64 on the expanded table, all-ones weights, the one-bag-per-lookup
    restatement that lets the unweighted fp32 oracle stand beside a weighted case, and the pooling dispatch thresholds."""
import os
import re

import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import tt_ref64 as R
from util import ATOL_SCALE, EPS, LR, adagrad_expected, assert_adagrad_close, assert_close, sgd_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")


def _ref(c, with_grad=True):
    rowidx, tableidx = R.rowidx_from_offsets(c["offsets"], c["tables"])
    return R.forward_backward(c["tables"], c["p"], c["q"], c["r"], c["B"], c["indices"], rowidx, tableidx, c["cores"],
                              c["d_out"] if with_grad else None)


@pytest.mark.parametrize("which", ["small_cases", "round4_cases"])
def test_reference_reproduces_the_goldens(which, request):
    """every golden case: outputs and gradients at atol 2e-6 max|ref| (no relative part; measured worst 6.4e-7), then the SGD and
    Adagrad steps tests/util.py expects from the golden gradients against the reference's own steps"""
    cases = request.getfixturevalue(which)
    assert len(cases) >= 5
    for name, c in cases.items():
        ref = _ref(c)
        assert_close(c["out"], ref["out"], f"{name} out", rtol=0.0, atol_scale=ATOL_SCALE)
        for k in range(c["T"]):
            assert_close(c["grads"][k], ref["grads"][k], f"{name} grad{k}", rtol=0.0, atol_scale=ATOL_SCALE)
            # a slice the batch does not touch has no gradient, in the goldens as in the reference
            m = R.slice_mask(ref["touched"], c["cores"])[k]
            assert not np.asarray(c["grads"][k])[~m].any() and not ref["grads"][k][~m].any(), f"{name} grad{k}: untouched slices"
        sgd = R.sgd_step(c["cores"], ref["grads"], LR)
        for k, e in enumerate(sgd_expected(c["cores"], c["grads"])):
            assert_close(e, sgd[k], f"{name} sgd core{k}")
        zero = [np.zeros_like(x) for x in c["cores"]]
        w, s = R.adagrad_step(c["cores"], zero, ref["grads"], ref["touched"], LR, EPS)
        exp_w, exp_s = adagrad_expected(c["cores"], c["grads"])
        for k in range(c["T"]):
            R.assert_state_close(exp_s[k], s[k], ref["grads"][k], f"{name} adagrad state{k}")
            assert_adagrad_close(exp_w[k], w[k], ref["grads"][k], f"{name} adagrad core{k}")


def _case(seed, T, tables, p, q, r, B, pf, std=2):
    r = G.pad_ranks(r, T)
    E_, D = int(np.prod(p)), int(np.prod(q))
    idx, off = G.make_bags(seed, B, E_, pf, std, tables)
    return dict(tables=tables, T=T, p=p, q=q, r=r, B=B, D=D, indices=idx, offsets=off,
                cores=G.make_cores(seed + 1, tables, p, q, r, "signed"), d_out=G.make_grad(seed + 2, tables, B, D))


@pytest.mark.parametrize("T,tables,p,q,r,B,pf", [
    (2, 1, [9, 8], [8, 8], [32], 120, 6),
    (2, 3, [7, 9], [3, 4], [13], 60, 5),
    (3, 1, [6, 5, 7], [4, 4, 4], [32, 32], 150, 8),
    (3, 4, [7, 9, 11], [3, 4, 5], [13, 12], 90, 5),
    (3, 2, [5, 6, 7], [3, 3, 5], [13, 11], 80, 6),
    (4, 1, [4, 5, 3, 4], [2, 4, 4, 2], [32, 32, 32], 100, 6),
    (4, 3, [7, 9, 11, 5], [3, 4, 5, 7], [13, 12, 7], 50, 4),
])
def test_oracle_agrees_with_the_reference(T, tables, p, q, r, B, pf):
    """forward, dense gradients, one SGD step and one Adagrad step from a live state: oracle/ttx_oracle.c (fp32, sequential) against
    the float64 reference at the default tolerance (a few thousand lookups over a few slices: the oracle's own rounding stays well
    inside it)"""
    c = _case(100 * T + tables, T, tables, p, q, r, B, pf)
    ref = _ref(c)
    g = O.make_geom(tables, p, q, c["r"])
    rowidx, tableidx = O.rowidx_from_offsets(c["offsets"], tables)
    what = f"T={T} tables={tables} q={q} r={r}"
    assert_close(O.tt_forward(g, B, c["D"], c["indices"], rowidx, tableidx, c["cores"]), ref["out"], what + " out")
    grads = O.tt_backward(g, O.OPTIM_DENSE, B, c["D"], 0, 0, c["indices"], rowidx, tableidx, c["d_out"], [x.copy() for x in c["cores"]])
    mask = R.slice_mask(ref["touched"], c["cores"])
    for k in range(T):
        assert_close(grads[k], ref["grads"][k], what + f" grad{k}")
        assert not grads[k][~mask[k]].any()
        assert 0 < ref["touched"][k].sum()
    for lr, eps in ((LR, EPS), (0.03, 1e-2)):
        w = [x.copy() for x in c["cores"]]
        O.tt_backward(g, O.OPTIM_SGD, B, c["D"], lr, 0, c["indices"], rowidx, tableidx, c["d_out"], w)
        for k, e in enumerate(R.sgd_step(c["cores"], ref["grads"], lr)):
            assert_close(w[k], e, what + f" sgd core{k} lr={lr}")
        state0, zeroed = R.live_state(ref["grads"], ref["touched"], 7 + T)
        w, s = [x.copy() for x in c["cores"]], [x.copy() for x in state0]
        O.tt_backward(g, O.OPTIM_ADAGRAD, B, c["D"], lr, eps, c["indices"], rowidx, tableidx, c["d_out"], w, s)
        ew, es = R.adagrad_step(c["cores"], state0, ref["grads"], ref["touched"], lr, eps)
        for k in range(T):
            assert ref["touched"][k][zeroed[k]] and not state0[k].reshape(ref["touched"][k].size, -1)[zeroed[k]].any()
            R.assert_state_close(s[k], es[k], ref["grads"][k], what + f" adagrad state{k}")
            assert_adagrad_close(w[k], ew[k], ref["grads"][k], what + f" adagrad core{k} lr={lr}", lr=lr, eps=eps, state0=state0[k])
            # untouched slices: the oracle leaves weights and state alone, bit for bit
            assert np.array_equal(w[k][~mask[k]], c["cores"][k][~mask[k]]) and np.array_equal(s[k][~mask[k]], state0[k][~mask[k]])


def test_reference_takes_tables_of_different_row_factors():
    """`p` per table: the cores are [1, sum p, slice]; equal to every table done on its own"""
    q, r, B = [2, 3, 2], [1, 4, 5, 1], 12
    ps = [[3, 4, 5], [6, 2, 3], [2, 2, 7]]
    rs = np.random.RandomState(3)
    per, idx, lens = [], [], []
    for k, pk in enumerate(ps):
        per.append(G.make_cores(30 + k, 1, pk, q, r, "signed"))
        n = rs.randint(0, 5, size=B)
        lens.append(n)
        idx.append(rs.randint(0, int(np.prod(pk)), size=int(n.sum())))
    off = np.concatenate([[0], np.cumsum(np.concatenate(lens))]).astype(np.int64)
    idx = np.concatenate(idx).astype(np.int64)
    cores = [np.concatenate([per[k][t] for k in range(3)], axis=1) for t in range(3)]
    d_out = G.make_grad(9, 3, B, 12)
    rowidx, tableidx = R.rowidx_from_offsets(off, 3)
    got = R.forward_backward(3, ps, q, r, B, idx, rowidx, tableidx, cores, d_out)
    for k in range(3):
        sel = tableidx == k
        one = R.forward_backward(1, ps[k], q, r, B, idx[sel], rowidx[sel], np.zeros(int(sel.sum()), dtype=np.int64), per[k], d_out[k:k + 1])
        assert np.allclose(got["out"][k], one["out"][0], rtol=1e-13, atol=0)
        for t in range(3):
            b = sum(pk[t] for pk in ps[:k])
            assert np.allclose(got["grads"][t][0, b:b + ps[k][t]], one["grads"][t][0], rtol=1e-13, atol=1e-300)


# ---- per_sample_weights ----------------------------------------------------------------------------------------------------------
def _forward_backward_before_weights(tables, p, q, r, B, indices, rowidx, tableidx, cores, d_out=None, block_doubles=1 << 23):
    """tt_ref64.forward_backward as it stood before it took per_sample_weights, kept word for word: what `None` must reproduce bit for bit"""
    g = R.Geometry(tables, p, q, r)
    T, rr, qq = g.T, g.r, g.q
    idx = np.asarray(indices, dtype=np.int64)
    row = np.asarray(rowidx, dtype=np.int64)
    tb = np.asarray(tableidx, dtype=np.int64)
    nnz = idx.size
    W = g.cores2d(cores)
    out = np.zeros((tables * B, g.D))
    grads = [np.zeros_like(w) for w in W] if d_out is not None else None
    touched = [np.zeros(g.S[t], dtype=bool) for t in range(T)]
    res = dict(out=out.reshape(tables, B, g.D), touched=touched)
    if d_out is not None:
        res["grads"] = [gr.reshape(np.asarray(c).shape) for gr, c in zip(grads, cores)]
    if nnz == 0:
        return res
    sid = g.slice_ids(idx, tb)
    for t in range(T):
        touched[t][sid[t]] = True
    bag = tb * B + row
    # distinct (table, index) pairs; `inv` maps a lookup onto its pair
    emax = int(np.prod(g.p_tables, axis=1).max())
    key, first, inv = np.unique(tb * emax + idx, return_index=True, return_inverse=True)
    U = key.size
    usid = [s[first] for s in sid]
    gU = None
    if d_out is not None:
        gU = np.zeros((U, g.D))
        np.add.at(gU, inv, np.asarray(d_out, dtype=np.float64).reshape(tables * B, g.D)[bag])
    rows = np.empty((U, g.D))
    blk = max(1, int(block_doubles // max(max(g.slice), g.D)))
    for u0 in range(0, U, blk):
        u1 = min(U, u0 + blk)
        n = u1 - u0
        G = [W[t][usid[t][u0:u1]].reshape(n, rr[t], qq[t], rr[t + 1]) for t in range(T)]
        # Left[t]: [n, q_0 .. q_{t-1}, r_t]
        left = [np.ones((n, 1, 1))]
        for t in range(T):
            nxt = np.matmul(left[t], G[t].reshape(n, rr[t], qq[t] * rr[t + 1]))          # [n, Ql, q_t r_{t+1}]
            left.append(nxt.reshape(n, -1, rr[t + 1]))
        rows[u0:u1] = left[T].reshape(n, g.D)
        if d_out is None:
            continue
        # Right[t]: [n, r_{t+1}, q_{t+1} .. q_{T-1}]
        right = [None] * T
        right[T - 1] = np.ones((n, 1, 1))
        for t in range(T - 1, 0, -1):
            prv = np.matmul(G[t].reshape(n, rr[t] * qq[t], rr[t + 1]), right[t])        # [n, r_t q_t, Qr]
            right[t - 1] = prv.reshape(n, rr[t], -1)
        for t in range(T):
            Ql, Qr = left[t].shape[1], right[t].shape[2]
            gg = gU[u0:u1].reshape(n, Ql, qq[t] * Qr)
            a = np.matmul(left[t].transpose(0, 2, 1), gg).reshape(n, rr[t] * qq[t], Qr)   # [n, r_t q_t, Qr]
            dG = np.matmul(a, right[t].transpose(0, 2, 1)).reshape(n, g.slice[t])         # [n, r_t q_t r_{t+1}]
            s = usid[t][u0:u1]
            order = np.argsort(s, kind="stable")
            ss = s[order]
            starts = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
            grads[t][ss[starts]] += np.add.reduceat(dG[order], starts, axis=0)
    np.add.at(out, bag, rows[inv])
    return res


@pytest.mark.parametrize("which", ["small_cases", "round4_cases"])
def test_reference_without_weights_is_bit_identical_to_before(which, request):
    """per_sample_weights=None: outputs, gradients and touched slices of every golden case bit for bit those of the reference's
    earlier text (with and without d_out)"""
    cases = request.getfixturevalue(which)
    for name, c in cases.items():
        rowidx, tableidx = R.rowidx_from_offsets(c["offsets"], c["tables"])
        args = (c["tables"], c["p"], c["q"], c["r"], c["B"], c["indices"], rowidx, tableidx, c["cores"])
        for d_out in (c["d_out"], None):
            new, old = R.forward_backward(*args, d_out, per_sample_weights=None), _forward_backward_before_weights(*args, d_out)
            assert sorted(new) == sorted(old), f"{name}: result keys {sorted(new)}"
            assert np.array_equal(new["out"], old["out"]), f"{name}: out"
            for k in range(c["T"]):
                assert np.array_equal(new["touched"][k], old["touched"][k]), f"{name}: touched {k}"
                assert d_out is None or np.array_equal(new["grads"][k], old["grads"][k]), f"{name}: grad {k}"


def _weights(seed, nnz):
    rs = np.random.RandomState(seed)
    w = (rs.rand(nnz) * 2.0 - 0.5).astype(np.float32)
    w[rs.rand(nnz) < 0.1] = 0.0
    return w


def _wcase(seed, T, tables, p, q, r, B, pf):
    """as _case, with a fifth of the bags empty and indices drawn from a tenth of the table (repeats within and across bags)"""
    c = _case(seed, T, tables, p, q, r, B, pf)
    rs = np.random.RandomState(seed + 3)
    lens = rs.randint(1, 2 * pf, size=tables * B) * (rs.rand(tables * B) > 0.2)
    c["offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    c["indices"] = (rs.randint(0, max(3, int(np.prod(p)) // 10), size=int(lens.sum())) * 7 % int(np.prod(p))).astype(np.int64)
    return c


WEIGHTED = [
    (2, 1, [9, 8], [8, 8], [32], 40, 4),
    (2, 3, [7, 9], [3, 4], [13], 30, 3),
    (3, 1, [6, 5, 7], [4, 4, 4], [16, 16], 50, 5),
    (3, 3, [7, 9, 11], [3, 4, 5], [13, 12], 30, 4),
    (4, 1, [4, 5, 3, 4], [2, 4, 4, 2], [32, 32, 32], 30, 4),
    (4, 3, [3, 4, 2, 3], [3, 4, 2, 3], [13, 12, 7], 25, 3),
]


@pytest.mark.parametrize("T,tables,p,q,r,B,pf", WEIGHTED)
def test_weighted_reference_against_torch_float64(T, tables, p, q, r, B, pf):
    """the table expanded by tt_matrix_to_full in float64, F.embedding_bag(mode="sum", per_sample_weights=) and autograd in float64:
    forward, the cores' gradients and the weights' own gradient, at 1e-12 of the largest value (two float64 computations)"""
    import tt_embeddings_ops as ops

    c = _wcase(300 * T + tables, T, tables, p, q, r, B, pf)
    nnz = c["indices"].size
    w = _weights(5 + T + tables, nnz)
    rowidx, tableidx = R.rowidx_from_offsets(c["offsets"], tables)
    assert (w == 0).any() and (np.diff(c["offsets"]) == 0).any() and np.unique(tableidx * 10 ** 6 + c["indices"]).size < nnz
    ref = R.forward_backward(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, c["cores"], c["d_out"], per_sample_weights=w)
    tc = [torch.tensor(x, dtype=torch.float64, requires_grad=True) for x in c["cores"]]
    tw = torch.tensor(w, dtype=torch.float64, requires_grad=True)
    outs = []
    for k in range(tables):
        full = ops.tt_matrix_to_full(p, q, c["r"], [x[k:k + 1] for x in tc], [1, 0, 2, 3])
        assert full.dtype == torch.float64 and tuple(full.shape) == (int(np.prod(p)), c["D"])
        # (float32 cores still give the float32 table they always gave: the float64 one rounded, up to fp32 rounding of the products)
        full32 = ops.tt_matrix_to_full(p, q, c["r"], [torch.from_numpy(x[k:k + 1]) for x in c["cores"]], [1, 0, 2, 3])
        assert full32.dtype == torch.float32 and full32.shape == full.shape
        assert_close(full32.numpy(), full.detach().numpy(), f"float32 table {k}")
        lo, hi = int(c["offsets"][k * B]), int(c["offsets"][(k + 1) * B])
        off = torch.from_numpy(c["offsets"][k * B:(k + 1) * B] - lo)
        outs.append(torch.nn.functional.embedding_bag(torch.from_numpy(c["indices"][lo:hi]), full, off, mode="sum",
                                                      per_sample_weights=tw[lo:hi]))
    out = torch.stack(outs)
    (out * torch.tensor(c["d_out"], dtype=torch.float64)).sum().backward()

    def same(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-300), f"{what}: {np.abs(a - b).max():.3e}"

    same(ref["out"], out.detach().numpy(), "out")
    for k in range(T):
        same(ref["grads"][k], tc[k].grad.numpy(), f"grad{k}")
    same(ref["d_psw"], tw.grad.numpy(), "d_psw")
    assert np.abs(ref["d_psw"][w == 0]).min() > 0, "a lookup of weight 0 still has a weight gradient"
    # all-ones weights: the unweighted results, bit for bit (1.0 x is x), and touched does not look at the weights
    plain = R.forward_backward(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, c["cores"], c["d_out"])
    ones = R.forward_backward(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, c["cores"], c["d_out"],
                              per_sample_weights=np.ones(nnz, dtype=np.float32))
    assert "d_psw" not in plain and np.array_equal(ones["out"], plain["out"])
    for k in range(T):
        assert np.array_equal(ones["grads"][k], plain["grads"][k])
        assert np.array_equal(ones["touched"][k], plain["touched"][k]) and np.array_equal(ref["touched"][k], plain["touched"][k])
    zero = R.forward_backward(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, c["cores"], c["d_out"],
                              per_sample_weights=np.zeros(nnz, dtype=np.float32))
    assert not zero["out"].any() and not any(x.any() for x in zero["grads"]) and np.array_equal(zero["d_psw"], ref["d_psw"])


@pytest.mark.parametrize("T,tables,p,q,r,B,pf", WEIGHTED)
def test_per_lookup_restatement_puts_the_oracle_beside_a_weighted_case(T, tables, p, q, r, B, pf):
    """one bag per lookup with d_out' = w d_out[bag]: the unweighted fp32 oracle's gradients, SGD step and -- rows pooled in fp32 --
    forward against the weighted float64 reference at the default tolerance"""
    c = _wcase(400 * T + tables, T, tables, p, q, r, B, pf)
    nnz, D = c["indices"].size, c["D"]
    w = _weights(9 + T + tables, nnz)
    rowidx, tableidx = R.rowidx_from_offsets(c["offsets"], tables)
    ref = R.forward_backward(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, c["cores"], c["d_out"], per_sample_weights=w)
    g = O.make_geom(tables, p, q, c["r"])
    rs = R.per_lookup_restatement(tables, B, rowidx, tableidx, w, c["d_out"])
    assert rs["B"] == nnz and np.array_equal(rs["rowidx"], np.arange(nnz)) and rs["d_out"].shape == (tables, nnz, D)
    assert np.count_nonzero(rs["d_out"].reshape(tables * nnz, D).any(axis=1)) == np.count_nonzero(w)
    rows = O.tt_forward(g, nnz, D, c["indices"], rs["rowidx"], tableidx, c["cores"])
    packed = R.oracle_on_restatement(tables, p, q, c["r"], B, c["indices"], rowidx, tableidx, w, c["cores"], c["d_out"], LR)
    out, d_psw = R.pool_per_lookup_fp32(tables, B, rowidx, tableidx, w, rows, c["d_out"])
    assert out.dtype == np.float32 and d_psw.dtype == np.float32
    assert np.array_equal(packed[0], out) and np.array_equal(packed[1], d_psw)
    assert_close(out, ref["out"], "restated out")
    assert_close(d_psw, ref["d_psw"], "restated d_psw")
    grads = O.tt_backward(g, O.OPTIM_DENSE, nnz, D, 0, 0, c["indices"], rs["rowidx"], tableidx, rs["d_out"], [x.copy() for x in c["cores"]])
    wts = [x.copy() for x in c["cores"]]
    O.tt_backward(g, O.OPTIM_SGD, nnz, D, LR, 0, c["indices"], rs["rowidx"], tableidx, rs["d_out"], wts)
    for k, e in enumerate(R.sgd_step(c["cores"], ref["grads"], LR)):
        assert_close(grads[k], ref["grads"][k], f"restated grad{k}")
        assert_close(wts[k], e, f"restated sgd core{k}")
        # (oracle_on_restatement: the same, rows per distinct pair and the SGD step taken from the dense gradients)
        assert np.array_equal(packed[2][k], grads[k]) and R.widen_factor(packed[3][k], e) == (1.0, R.default_units(packed[3][k], e))
    # (and the restatement of an unweighted batch -- all ones -- is the oracle on the batch itself, up to the order of its sums)
    plain = O.tt_forward(g, B, D, c["indices"], rowidx, tableidx, c["cores"])
    assert_close(R.pool_per_lookup_fp32(tables, B, rowidx, tableidx, np.ones(nnz), rows)[0], plain, "all-ones restatement")


def test_pooling_dispatch_thresholds_match_the_sources():
    """tests/tt_ref64.py::pool_route restates which pooling kernel ttx_tt_forward_o takes (the cases of
    tests/test_per_sample_weights_gpu.py are named for them); a retune of kPoolSpanMin or of the dispatch must fail HERE"""
    tt = open(os.path.join(CSRC, "ttx_tt.hip")).read()
    spec = open(os.path.join(CSRC, "ttx_tt_spec.inc")).read()
    assert int(_constexpr(tt, "kPoolSpanMin")) == R.POOL_SPAN_MIN
    assert _define(spec, "TTX_MC32") == R.SPEC_MC32 and _code("using S_32_4_32_4 = Shape3<32, 4, 32, 4, TTX_NP32, TTX_MC32>;") in _code(spec)
    tt, spec = _code(tt), _code(spec)
    # the shapes whose backward reads the bag gradient per column pass (Shape3::GPP: the weight goes through L.gsw there), and the
    # D = 1024 template the GPU file's case for them uses
    assert _code("static constexpr bool GPP = TTX_GPP && (R1_ == 64 || Q0_ * Q1_ * Q2_ >= 1024) && Q0_ == 4 && NP_ > 1;") in spec
    assert _code("using S_32_16_32_16 = Shape3<32, 16, 32, 16, 8, 16>;") in spec and _code("#define TTX_GPP 1") in spec
    # the two-core kernel's shapes (everything else with two cores stays on the generic kernels: bwd_load_dx0), and the generic
    # backward's loads of the bag gradients by D % 4 -- the GPU file's generic cases restate these
    assert _code("return d.T == 2 && !g_disable_spec && d.r[1] <= 128 && d.q[0] <= 32 && d.q[1] <= 32 && d.r[1] * d.q[1] <= 2048;") in tt
    gen = _code(open(os.path.join(CSRC, "ttx_tt_generic.inc")).read())
    assert gen.count(_code("if (d.T == 2) { bwd_load_dx0(d, L, smem, B, table, rowidx, d_output, PC,")) == 2
    assert _code("float* Gb = smem + L.oG; if ((D & 3) == 0) {") in gen
    # a plan chunk longer than the template's is walked in sub-chunks
    assert spec.count(_code("if (P.MC > S::MC)")) == 2
    # fused pooling is OFFERED to the specialised kernels ...
    assert _code("const bool offer = offsets && arrive && nnz <= kPoolSpanMin && d.D % 4 == 0 &&") in tt
    # ... which take it when the shape is unpadded, not sub-chunked, and D % 4 == 0
    assert _code("if (pad) return spec_launch_fwd_v<S, false, false, true>(P, C, rows, zout, nzero, F, R, st); "
                 "if constexpr (S::D % 4 == 0) { if (want) { *fused = true;") in spec
    # the pooling launch otherwise: float4 small / float4 large / scalar
    assert _code("} else if (!(g_skip_launch & 1) && !fused) {") in tt
    assert _code("if (d.D % 4 == 0 && (((uintptr_t)rows | (uintptr_t)output) & 15) == 0) { "
                 "if (nnz <= kPoolSpanMin && (unsigned long long)nnz * d.D * 4 < (1ull << 32) - 16) hipLaunchKernelGGL(pool4_small_kernel,") in tt
    assert _code("else hipLaunchKernelGGL(pool4_kernel,") in tt and _code("} else { const int groups = kThreads / 32; hipLaunchKernelGGL(pool_kernel,") in tt
    # the dedup route's pooling: gather4 beyond kPoolSpanMin, else float4 / float by D % 4
    assert _code("& 15) == 0 && nnz > kPoolSpanMin) hipLaunchKernelGGL(pool_gather4_kernel,") in tt
    assert R.pool_route(300, 64, True, True) == "fused" and R.pool_route(300, 64, False, True) == "pool4_small"
    assert R.pool_route(300, 60, True, True, padded=True) == "pool4_small" and R.pool_route(300, 45, True, True) == "pool_scalar"
    assert R.pool_route(65536, 64, False, True) == "pool4_small" and R.pool_route(65537, 64, True, True) == "pool4"
    assert R.pool_route(300, 60, True, False) == "pool4_small" and R.pool_route(70000, 45, False, False) == "pool_scalar"


# ---- the apply-site classifier ---------------------------------------------------------------------------------------------------
def _define(text, name):
    m = re.search(r"#define\s+" + name + r"\s+(\d+)\b", text)
    assert m, f"#define {name} not found"
    return int(m.group(1))


def _constexpr(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, f"constexpr int {name} not found"
    return m.group(1).strip()


def _code(text):
    """program text without comments and white space"""
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"\s+", "", text)


def test_classifier_constants_match_the_sources():
    """tests/tt_ref64.py mirrors the thresholds that decide which apply site a slice takes.  A retune of one of them must fail HERE:
    otherwise the cases of tests/test_fused_optimizer_gpu.py would quietly stop reaching the site they are named for."""
    internal = open(os.path.join(CSRC, "ttx_internal.h")).read()
    tt = open(os.path.join(CSRC, "ttx_tt.hip")).read()
    plan = open(os.path.join(CSRC, "ttx_plan.hip")).read()
    assert _define(internal, "TTX_SEG_THIN") == R.SEG_THIN
    assert _define(internal, "TTX_HOT_PIVOT") == R.HOT_PIVOT
    assert _constexpr(internal, "kSegThin") == "TTX_SEG_THIN" and _constexpr(internal, "kHotRowsPivot") == "TTX_HOT_PIVOT"
    assert _define(tt, "TTX_MAX_HOT_PIVOT") == R.MAX_HOT_PIVOT and _constexpr(tt, "kMaxHotPivot") == "TTX_MAX_HOT_PIVOT"
    assert int(_constexpr(tt, "kSegPivot")) == R.SEG_PIVOT
    kwave = int(_constexpr(internal, "kWave"))
    assert int(_constexpr(plan, "kMbFuseU")) * 4096 == R.PLAN_UNITS_MAX_NNZ
    # (from here on EXPRESSIONS, compared without comments and white space: a reworded comment or a reformat is no retune)
    tt, plan = _code(tt), _code(plan)
    # the pack condition ("a wave per slice, four per work-group")
    m = re.search(r"smax<=(\d+)\*kWave&&smin4==0&&nslices>=(\d+)&&!g_no_pack", tt)
    assert m, "the pack condition of reduce_apply's launch has changed: update tests/tt_ref64.py::classify_apply_sites"
    assert int(m.group(1)) * kwave == R.PACK_MAX_FLOATS and int(m.group(2)) == R.PACK_MIN_SLICES
    # a slice is hot at MORE than kHotRowsPivot chunk partials (pivot) / 2 segments of lookups (thin): owner, packed owner
    hot = "end - beg > (t == 1 ? kHotRowsPivot : 2 * seg_len(t)) && PC.hot_cnt && !(t == 1 && P.hdr[8 + 1] > kMaxHotPivot)"
    assert tt.count(_code(hot)) == 2, "the owners' hot-slice test has changed"
    assert _code("seg_len(int t) { return t == 1 ? kSegPivot : kSegThin; }") in tt
    assert _code("if (t == 1 && P.hdr[8 + 1] > kMaxHotPivot) return;") in tt
    assert _code("if ((sl & 3) != 0) return;") in tt  # (odd slice sizes stay with their single owner)
    assert _code("return (sl & 3) ? 0 : (sl / 4 + kHotColsPivot - 1) / kHotColsPivot;") in tt
    # the plans that COUNT the hot pivot slices (the others leave "some": the column split whatever their number)
    assert _code("P.hdr[8 + 1] = wt[0] ? -1 : 0;") in plan and _code("if (dg == 0) hdr[8 + 1] = nhot;") in plan
    assert _code("__syncthreads_count(nf + np > kHotRowsPivot)") in plan and _code("tot > 2 * kSegThin") in plan
    assert _code("nnz > 1024 || !d.idx32 || n_dev") in plan and R.PLAN_TINY_NNZ == 1024
    assert _code("maxp == 1 && N <= kOneMaxN && !d.tab") in plan and R.PLAN_ONE_DIGIT == 256


def _idx(p, digits):
    """indices from per-core digit arrays"""
    idx = np.zeros(len(digits[0]), dtype=np.int64)
    for t, d in enumerate(digits):
        idx = idx * p[t] + np.asarray(d, dtype=np.int64)
    return idx


def test_classifier_on_hand_made_batches():
    p, q, r = [4, 6, 5], [4, 4, 4], [1, 16, 16, 1]
    n = 512 + 513 + 100
    d0 = np.repeat([0, 1, 3], [512, 513, 100])             # 512 lookups: not hot; 513: hot; slice 2 untouched
    d1 = np.repeat([0, 1, 2], [16 * 32, 16 * 32 + 1, n - 1025])  # 16 chunk partials at mc = 32: not hot; 17: hot
    d2 = np.arange(n) % 5
    c = R.classify_apply_sites(_idx(p, [d0, d1, d2]), np.zeros(n, dtype=np.int64), 1, p, q, r, mc=32)
    assert c["cores"][0]["thin_fold"] == 1 and c["cores"][0]["float4_owner"] == 2 and sum(c["cores"][0].values()) == 3
    assert c["cores"][1]["pivot_columns"] == 1 and c["cores"][1]["float4_owner"] == 2 and c["pivot_count_known"] and not c["pack"]
    assert c["cores"][2]["float4_owner"] == 5 and c["rows"][1].tolist()[:3] == [16, 17, 4]
    # more hot pivot slices than kMaxHotPivot, counted by the plan: their owners keep them
    p9 = [3, 12, 3]
    n9 = 10 * 600
    d1 = np.repeat(np.arange(10), 600)
    c = R.classify_apply_sites(_idx(p9, [np.arange(n9) % 3, d1, np.arange(n9) % 2]), np.zeros(n9, dtype=np.int64), 1, p9, q, r, mc=32)
    assert c["cores"][1]["pivot_owner_fallback"] == 10 and c["cores"][1]["pivot_columns"] == 0
    assert c["cores"][0]["thin_fold"] == 3 and c["cores"][2]["thin_fold"] == 2 and c["cores"][2]["float4_owner"] == 0
    # (table ids beyond one digit: the wide-digit plan leaves "some", the column split takes them all)
    c = R.classify_apply_sites(_idx(p9, [np.arange(n9) % 3, d1, np.arange(n9) % 2]), np.full(n9, 29, dtype=np.int64), 30, p9, q, r, mc=32)
    assert not c["pivot_count_known"] and c["cores"][1]["pivot_columns"] == 10
    # odd slice sizes: the scalar owner, hot or not; many small slices: packed; two hot slices meeting in one segment
    c = R.classify_apply_sites(_idx([5, 6, 7], [np.zeros(700), np.arange(700) % 6, np.arange(700) % 7]), np.zeros(700, dtype=np.int64), 1,
                               [5, 6, 7], [3, 3, 5], [1, 13, 11, 1], mc=16)
    assert [x["scalar_owner"] for x in c["cores"]] == [1, 6, 7] and sum(sum(x.values()) for x in c["cores"]) == 14
    pk = [400, 500, 450]
    d0 = np.repeat([7, 8, 9, 300], [600, 700, 5, 1])
    c = R.classify_apply_sites(_idx(pk, [d0, np.arange(1306) % 400, np.arange(1306) % 450]), np.zeros(1306, dtype=np.int64), 1, pk,
                               [4, 4, 4], [1, 4, 4, 1], mc=32)
    assert c["pack"] and c["cores"][0]["thin_fold"] == 2 and c["cores"][0]["packed"] == 2 and c["shared_segments"][0] == 1
    assert c["cores"][1]["packed"] == 400 and c["cores"][0]["float4_owner"] == 0
    # four cores on the three-core kernels: cores 2 and 3 belong to t4_apply23_kernel
    p4 = [4, 5, 3, 4]
    i4 = np.arange(240) % 240
    c = R.classify_apply_sites(i4, np.zeros(240, dtype=np.int64), 1, p4, [2, 4, 4, 2], [1, 32, 32, 32, 1], mc=32, merged_last_cores=True)
    assert c["cores"][2]["t4_apply23"] == 3 and c["cores"][3]["t4_apply23"] == 4 and c["cores"][0]["float4_owner"] == 4
