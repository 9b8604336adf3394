"""The reference's OWN module code, pinned through its recorded behaviour (round-5 verdict item 6).  Nothing of
the reference is copied: tests/golden/ref_cache_life_cycle.{json,npz} hold what the reference's TTEmbeddingBag did -- the calls it
made into its native module and the numbers it returned -- when tests/run_reference_tests.py drove it through a cache life cycle
recorded where the reference tree lies, in an empty directory, with REPO the repository's root:
    TTX_TRACE_NPZ=$REPO/tests/golden/ref_cache_life_cycle.npz python $REPO/tests/run_reference_tests.py --trace \
        > $REPO/tests/golden/ref_cache_life_cycle.json
The reference's six property tests themselves (tt_embeddings_test.py) need its tree: `python tests/run_reference_tests.py` runs
them on the oracle by hand; the vectors they derive from are pinned by tests/golden/small_cases.npz (tests/test_oracle_golden.py)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")


def test_call_order_and_results_of_a_cache_life_cycle_match_the_references_module(monkeypatch):
    """Rows a2 / a14: the reference's TTEmbeddingBag (its own Python, ops.py:421-934) and the product's, driven through the same
    cache life cycle on the same stand-in engine -- counting steps, cache_populate, cache-live steps; fused SGD, fused Adagrad,
    dense -- make the SAME sequence of native-module calls (names, scalar arguments, tensor shapes and dtypes, positional order)
    and return the same numbers: outputs, cores, cache rows, dense gradients."""
    with open(os.path.join(GOLDEN, "ref_cache_life_cycle.json")) as f:
        ref_trace = json.loads(f.read().strip().splitlines()[-1])
    ref_results = np.load(os.path.join(GOLDEN, "ref_cache_life_cycle.npz"))
    import torch

    import oracle_engine
    import run_reference_tests as R
    import tt_embeddings_ops as ops

    monkeypatch.setattr(ops, "_engine", oracle_engine)
    for name in ("tt_forward", "tt_dense_backward", "tt_sgd_backward", "tt_adagrad_backward", "update_cache_state", "cache_populate",
                 "preprocess_indices_sync", "cache_forward", "cache_backward_sgd", "cache_backward_dense",
                 "cache_backward_rowwise_adagrad_approx"):
        monkeypatch.setattr(oracle_engine, name, getattr(oracle_engine, name))  # (life_cycle wraps them: restored afterwards)
    trace, results = R.life_cycle(ops, oracle_engine, torch, extra_kwargs=dict(device=torch.device("cpu")))
    trace = json.loads(json.dumps(trace))
    names = [e[0] for e in trace]
    assert names == [e[0] for e in ref_trace], "sequence of native-module calls"
    assert len(trace) == len(ref_trace) and sum(not e[0].startswith("--") for e in trace) > 40
    for mine, theirs in zip(trace, ref_trace):
        if mine[0].startswith("--"):
            continue
        assert len(mine[1]) == len(theirs[1]), f"{mine[0]}: number of positional arguments"
        for k, (x, y) in enumerate(zip(mine[1], theirs[1])):
            assert x == y, f"{mine[0]} positional argument {k}: {x} vs the reference's {y}"
        assert mine[2] == theirs[2] == [], f"{mine[0]}: keyword arguments {mine[2]} (the reference passes none)"
    assert len(results) == len(ref_results.files)
    for k, got in enumerate(results):
        want = ref_results[f"arr_{k}"]
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-7, err_msg=f"result {k}")
