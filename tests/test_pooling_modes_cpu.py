"""CPU tests (no GPU) of nn.EmbeddingBag's mean / max pooling modes on the TT bags: the constructor keyword, what it refuses,
state_dict keys, pickling, and the new C-ABI entry points (declared in include/ttx.h, exported by both libraries)."""
import copy
import ctypes
import os
import pickle
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ttx_bag_mean_scale", "ttx_tt_rows_p", "ttx_bag_max_pool", "ttx_bag_max_pool_backward",
               "ttx_tt_backward_rows_workspace_bytes", "ttx_tt_backward_rows")
P, Q, R = [5, 8], [3, 4], [6]


def small(ops, **kw):
    return ops.TTEmbeddingBag(40, 12, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", **kw)


def test_mode_keyword_validation():
    import tt_embeddings_ops as ops

    for mode in ops.POOLING_MODES:
        assert small(ops, mode=mode).mode == mode
    assert small(ops).mode == "sum"
    for bad in ("avg", "Sum", "", None, "min"):
        with pytest.raises(ValueError):
            small(ops, mode=bad)
    with pytest.raises(NotImplementedError):
        ops.TTEmbeddingBag(40, 12, R, P, Q, use_cache=True, cache_size=4, hashtbl_size=16, weight_dist="uniform",
                           device="cpu", mode="max")
    for dd in (True, "auto"):
        with pytest.raises(NotImplementedError):
            small(ops, mode="max", dedup=dd)
    # mean takes every option sum takes
    ops.TTEmbeddingBag(40, 12, R, P, Q, use_cache=True, cache_size=4, hashtbl_size=16, weight_dist="uniform", device="cpu",
                       mode="mean", dedup=True)
    tb = ops.TableBatchedTTEmbeddingBag(3, 40, 12, R, P, Q, weight_dist="uniform", device="cpu", mode="max")
    assert tb.mode == "max"
    with pytest.raises(ValueError):
        ops.TableBatchedTTEmbeddingBag(3, 40, 12, R, P, Q, weight_dist="uniform", device="cpu", mode="median")


def test_state_dict_keys_do_not_depend_on_mode():
    import tt_embeddings_ops as ops

    for kw in (dict(use_cache=False), dict(use_cache=True, cache_size=4, hashtbl_size=16)):
        for opt in (ops.OptimType.SGD, ops.OptimType.EXACT_ADAGRAD):
            keys = {}
            for mode in ops.POOLING_MODES:
                if mode == "max" and kw["use_cache"]:
                    continue
                m = ops.TTEmbeddingBag(40, 12, R, P, Q, weight_dist="uniform", device="cpu", optimizer=opt, mode=mode, **kw)
                keys[mode] = sorted(m.state_dict().keys())
            assert all(k == keys["sum"] for k in keys.values()), keys


def test_modules_pickle_and_deepcopy_with_their_mode():
    import tt_embeddings_ops as ops

    for mode in ops.POOLING_MODES:
        m = small(ops, mode=mode)
        assert copy.deepcopy(m).mode == mode
        assert pickle.loads(pickle.dumps(m)).mode == mode
        m2 = small(ops)
        m2.load_state_dict(m.state_dict())  # (same keys: a checkpoint moves between modes)


def test_module_without_mode_attribute_pools_by_sum():
    """a module pickled before the keyword existed has no `mode` attribute: it keeps the sum route"""
    import tt_embeddings_ops as ops

    m = small(ops)
    del m.__dict__["mode"]
    assert m.__dict__.get("mode", "sum") == "sum"


def test_new_entry_points_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "ttx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(ttx_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW_SYMBOLS) <= declared, set(NEW_SYMBOLS) - declared
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        missing = [s for s in NEW_SYMBOLS if not hasattr(lib, s)]
        assert not missing, f"{so} lacks {missing}"


def test_backward_rows_workspace_query():
    """host-only: the per-lookup-gradient backward needs the backward's workspace plus the positions (nnz int64)"""
    import tt_embeddings as E

    L = E.lib()
    for p, q, r in (([200, 220, 250], [4, 4, 4], [1, 32, 32, 1]), ([5, 8], [3, 4], [1, 6, 1]),
                    ([4, 5, 3, 4], [4, 4, 4, 4], [1, 32, 32, 32, 1])):
        g = E._geom(1, p, q, r)
        D = 1
        for v in q:
            D *= v
        for nnz in (1, 10240, 327680):
            base = L.ttx_tt_backward_workspace_bytes(ctypes.byref(g), 0, D, nnz)
            rows = L.ttx_tt_backward_rows_workspace_bytes(ctypes.byref(g), D, nnz)
            assert base > 0 and rows >= base + 8 * nnz
    bad = type(g)()
    bad.T = 7
    assert L.ttx_tt_backward_rows_workspace_bytes(ctypes.byref(bad), 4, 10) == 0


def test_pooling_entry_points_reject_bad_arguments_without_a_gpu():
    """argument checks run before anything touches a device"""
    import tt_embeddings as E

    L = E.lib()
    assert L.ttx_bag_mean_scale(-1, 4, None, None, None, None) == -1
    assert L.ttx_bag_mean_scale(3, 0, None, None, None, None) == -1
    assert L.ttx_bag_mean_scale(0, 4, None, None, None, None) == 0  # (nothing to do)
    assert L.ttx_bag_max_pool(2, 4, 10, None, None, None, None, None) == -1  # NULL inputs
    assert L.ttx_bag_max_pool(2, 4, 1 << 31, None, None, None, None, None) == -1
    assert L.ttx_bag_max_pool_backward(2, 4, 10, None, None, None, None, None) == -1
    assert L.ttx_bag_max_pool_backward(2, 4, 0, None, None, None, None, None) == 0
