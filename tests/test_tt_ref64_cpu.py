"""CPU tests of the float64 TT reference (tests/tt_ref64.py) and of the apply-site classifier beside it:
  * the reference against the golden vectors made by the reference project's own Python (outputs, gradients, and the SGD / Adagrad
    expectations tests/util.py derives from them);
  * the fp32 oracle (oracle/ttx_oracle.c) against the reference in all four modes, Adagrad from a live state: the two CPU
    restatements pinned to each other;
  * the classifier's mirrored thresholds against the library's sources, and the classifier on hand-made batches."""
import os
import re

import numpy as np
import pytest

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
