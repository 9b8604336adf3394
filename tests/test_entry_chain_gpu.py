"""The single-sub-chunk contraction kernels after their entry chain was shortened (csrc/ttx_tt_spec.inc: the arguments in one
round of the scalar cache with the chunk record, the table of a pivot slice from the host's magic pair instead of a division,
the first core_1 block requested with the lookup records).  Nothing arithmetic moved, so the results must be the bits the
kernels gave before.

Cases (tests/entry_chain_cases.py): p = [3, 4, 5], q = [4, 4, 4], ranks [32, 32]; chunks of 1, 4, 5 and 16 lookups, a pivot
slice of 17, one empty pivot slice per table, an empty bag per table; one table and three (table = s / p_1 = 0, 1, 2); with and
without per_sample_weights; a plan that carries bag rows and one that does not; forward, dense gradients, fused SGD.  Checked:
  1. forward output, dense gradients and the cores after the SGD step against the float64 reference (tests/tt_ref64.py) at the
     default tolerance (util.assert_close);
  2. a second run gives the same bits;
  3. the bits are those of tests/golden/entry_chain_t<tables>.npz, recorded from the commit before the change;
  4. the forward that pools the bags itself (offsets given: the fused-pooling variant, whose table of a pivot slice is the same
     magic pair, per lane) gives the recorded output too."""
import numpy as np
import pytest

import entry_chain_cases as EC
import tt_ref64 as R64
from util import assert_close

pytestmark = pytest.mark.gpu

_ref = {}


def reference(tables, case, cores, weighted):
    """float64 results of a case, computed once"""
    key = (tables, weighted)
    if key not in _ref:
        rowidx, tableidx = R64.rowidx_from_offsets(case["offsets"], tables)
        res = R64.forward_backward(tables, EC.P, EC.Q, EC.R, EC.B, case["indices"], rowidx, tableidx, cores, d_out=case["d_out"],
                                   per_sample_weights=case["psw"] if weighted else None)
        res["sgd"] = R64.sgd_step(cores, res["grads"], EC.LR)
        _ref[key] = res
    return _ref[key]


@pytest.mark.parametrize("tables", [1, 3])
def test_cases_force_the_chunk_lengths(tables):
    import tt_embeddings as E

    case = EC.make_case(tables)
    gold = np.load(EC.golden_path(tables))
    for k in ("indices", "offsets", "psw", "d_out"):
        assert np.array_equal(case[k], gold[k]), f"{k}: the generated case is not the recorded one"
    assert [EC.sha(c) for c in EC.make_cores(tables)] == list(gold["cores_sha"]), "the generated cores are not the recorded ones"
    rowidx, tableidx = R64.rowidx_from_offsets(case["offsets"], tables)
    lens = EC.pivot_lengths(tables, case["indices"], tableidx)
    assert lens.tolist() == EC.LENS[tables]
    chunks = sorted(set(min(EC.MC, n - c) for n in lens.ravel() for c in range(0, n, EC.MC)))
    assert chunks == [1, 4, 5, 16] and 17 in lens and (lens == 0).any(axis=1).all()
    assert (np.diff(case["offsets"]) == 0).sum() == tables
    assert sorted(set(tableidx.tolist())) == list(range(tables))
    assert E.debug_plan_layout(tables, EC.P, EC.Q, EC.R, int(case["indices"].size))["MC"] == EC.MC


@pytest.mark.parametrize("plan_rows", [True, False], ids=["rows", "norows"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("tables", [1, 3])
def test_results_are_the_parents_bits(tables, weighted, plan_rows):
    import tt_embeddings as E

    case, cores = EC.make_case(tables), EC.make_cores(tables)
    gold = np.load(EC.golden_path(tables))
    what = f"{tables} table(s), {'weighted' if weighted else 'plain'}, plan {'with' if plan_rows else 'without'} bag rows"
    out, grads, new = EC.run(E, tables, case, cores, weighted, plan_rows)
    # 1. float64
    ref = reference(tables, case, cores, weighted)
    assert_close(out, ref["out"], f"{what}: forward output")
    for k in range(3):
        assert_close(grads[k], ref["grads"][k], f"{what}: dense gradient of core {k}")
        assert_close(new[k], ref["sgd"][k], f"{what}: core {k} after the SGD step")
        assert not np.array_equal(new[k], cores[k]), f"{what}: the SGD step left core {k} alone"
    # 2. run to run
    out2, grads2, new2 = EC.run(E, tables, case, cores, weighted, plan_rows)
    assert np.array_equal(out, out2), f"{what}: forward output differs run to run"
    for k in range(3):
        assert np.array_equal(grads[k], grads2[k]) and np.array_equal(new[k], new2[k]), f"{what}: core {k} differs run to run"
    # 3. the recorded bits
    w = f"w{int(weighted)}"
    assert np.array_equal(out, gold[w + "_out"]), f"{what}: forward output is not the recorded one"
    assert [EC.sha(g) for g in grads] == list(gold[w + "_grad_sha"]), f"{what}: dense gradients are not the recorded ones"
    assert [EC.sha(c) for c in new] == list(gold[w + "_sgd_sha"]), f"{what}: cores after the SGD step are not the recorded ones"


@pytest.mark.parametrize("plan_rows", [True, False], ids=["rows", "norows"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("tables", [1, 3])
def test_fused_pooling_forward_gives_the_parents_bits(tables, weighted, plan_rows):
    import tt_embeddings as E

    case, cores = EC.make_case(tables), EC.make_cores(tables)
    gold = np.load(EC.golden_path(tables))
    assert R64.pool_route(int(case["indices"].size), EC.D, True, True) == "fused"
    what = f"{tables} table(s), {'weighted' if weighted else 'plain'}, plan {'with' if plan_rows else 'without'} bag rows, offsets given"
    out, _, _ = EC.run(E, tables, case, cores, weighted, plan_rows, offsets=True)
    assert_close(out, reference(tables, case, cores, weighted)["out"], f"{what}: forward output")
    assert np.array_equal(out, gold[f"w{int(weighted)}_out"]), f"{what}: forward output is not the recorded one"
    assert (out.reshape(-1, EC.D)[np.diff(case["offsets"]) == 0] == 0).all(), f"{what}: an empty bag is not zeros"
