"""CPU tests (no GPU) of nn.EmbeddingBag's padded batches on the TT bags: the `padding_idx` keyword, the 2-D fixed-length
input, the C ABI of ttx_bags_compact (declared, exported, argument checks) and, on top of the oracle engine (mode="sum"), the
module against torch's own embedding_bag(padding_idx=) on the expanded table."""
import copy
import ctypes
import os
import pickle
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_engine
from util import LR, assert_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, Q, R = [7, 9, 11], [3, 4, 5], [13, 12]
E_, D_ = 7 * 9 * 11, 60
PAD = 5


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", oracle_engine)
    return m


def single(ops, **kw):
    kw.setdefault("sparse", False)
    torch.manual_seed(3)
    return ops.TTEmbeddingBag(E_, D_, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", **kw)


def twin(ops, src, **kw):
    m = single(ops, **kw)
    with torch.no_grad():
        for a, b in zip(m.tt_cores, src.tt_cores):
            a.copy_(b)
    return m


# ------------------------------------------------------------------------------------------------------------ the keyword
def test_padding_idx_keyword_follows_torch(ops):
    assert single(ops).padding_idx is None
    assert single(ops, padding_idx=None).padding_idx is None
    assert single(ops, padding_idx=0).padding_idx == 0
    assert single(ops, padding_idx=E_ - 1).padding_idx == E_ - 1
    assert single(ops, padding_idx=-1).padding_idx == E_ - 1
    assert single(ops, padding_idx=-E_).padding_idx == 0
    assert single(ops, padding_idx=np.int64(7)).padding_idx == 7
    for bad in (E_, -E_ - 1, 1.5, "3", True):
        with pytest.raises(ValueError):
            single(ops, padding_idx=bad)
    tb = ops.TableBatchedTTEmbeddingBag(3, E_, D_, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", padding_idx=-2)
    assert tb.padding_idx == E_ - 2  # (one value, the same in every table)
    with pytest.raises(ValueError):
        ops.TableBatchedTTEmbeddingBag(3, E_, D_, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", padding_idx=E_)
    # torch's own modules agree on the accepted range and the normalisation
    assert torch.nn.EmbeddingBag(E_, 4, padding_idx=-1).padding_idx == E_ - 1
    with pytest.raises(AssertionError):
        torch.nn.EmbeddingBag(E_, 4, padding_idx=E_)


def test_padding_idx_survives_pickle_and_deepcopy_and_is_not_state(ops):
    m = single(ops, padding_idx=-3)
    assert copy.deepcopy(m).padding_idx == E_ - 3
    assert pickle.loads(pickle.dumps(m)).padding_idx == E_ - 3
    assert list(m.state_dict()) == list(single(ops).state_dict())
    # a module pickled before the keyword existed has no such attribute: it behaves as padding_idx=None
    old = single(ops)
    del old.__dict__["padding_idx"]
    idx, off = torch.tensor([PAD, 3, 9, PAD]), torch.tensor([0, 2, 4])
    ref = single(ops)
    assert torch.equal(old(idx, off), ref(idx, off))
    assert old.prefetch(idx, off) is False  # (CPU tensors: nothing planned ahead, and no attribute error on the way)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_bags_compact_is_declared_and_exported_and_checks_its_arguments():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ttx.h")).read(), flags=re.S)
    for name in ("ttx_bags_compact", "ttx_bags_compact_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr), f"{name} is not declared in include/ttx.h"
    i64, vp, sz = ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(ROOT, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        wsb, f = lib.ttx_bags_compact_workspace_bytes, lib.ttx_bags_compact
        wsb.restype, wsb.argtypes = sz, [i64, i64]
        f.argtypes = [i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, sz, vp]
        assert wsb(512, 20480) >= 4 * 20481
        assert wsb(16384, 655360) >= 4 * 655361
        # nothing to compact: 0, and with no buffers nothing touches a device
        assert f(0, 0, None, None, 0, 0, None, None, None, None, 0, None) == 0
        assert f(7, 0, None, None, 0, 0, None, None, None, None, 0, None) == 0
        # bad arguments: -1 with a message, before anything is launched (the pointers below are never dereferenced)
        fake = ctypes.c_void_p(4096)
        big = wsb(4, 40)
        for args in ((-1, 40, fake, None, 10, 0, fake, fake, fake, fake, big, None),        # negative nb
                     (4, -1, fake, None, 10, 0, fake, fake, fake, fake, big, None),         # negative nnz
                     (4, 1 << 31, fake, fake, 0, 0, fake, fake, fake, fake, 1 << 40, None),  # nnz >= 2^31
                     (4, 40, fake, None, 9, 0, fake, fake, fake, fake, big, None),          # offsets == NULL, nnz != nb * L
                     (4, 40, fake, None, -10, 0, fake, fake, fake, fake, big, None),        # negative L
                     (4, 40, None, None, 10, 0, fake, fake, fake, fake, big, None),         # NULL indices
                     (4, 40, fake, None, 10, 0, None, fake, fake, fake, big, None),         # NULL out_indices
                     (4, 40, fake, None, 10, 0, fake, None, fake, fake, big, None),         # NULL out_offsets
                     (4, 40, fake, None, 10, 0, fake, fake, None, fake, big, None),         # NULL n_live
                     (4, 40, fake, None, 10, 0, fake, fake, fake, None, big, None),         # NULL workspace
                     (4, 40, fake, None, 10, 0, fake, fake, fake, fake, big - 1, None)):    # workspace too small
            assert f(*args) == -1, args
            assert b"bags_compact" in lib.ttx_last_error(), lib.ttx_last_error()


def test_engine_exposes_bags_compact():
    import tt_embeddings as E

    assert callable(E.bags_compact)
    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.bags_compact(torch.zeros(4, dtype=torch.int64), None, 2, 0)


# ---------------------------------------------------------------------------------------------- the module, oracle engine
def test_2d_input_equals_the_flattened_1d_call_bit_for_bit(ops):
    rs = np.random.RandomState(1)
    idx = torch.from_numpy(rs.randint(0, E_, size=(6, 5)).astype(np.int64))
    d = torch.from_numpy(rs.standard_normal((6, D_)).astype(np.float32))
    for ilo in (True, False):
        a, b = single(ops, include_last_offset=ilo), None
        b = twin(ops, a, include_last_offset=ilo)
        off = torch.arange(0, 31, 5)
        oa = a(idx)
        ob = b(idx.reshape(-1), off if ilo else off[:-1])
        assert oa.shape == (6, D_) and torch.equal(oa, ob)
        oa.backward(d)
        ob.backward(d)
        for k in range(3):
            assert torch.equal(a.tt_cores[k].grad, b.tt_cores[k].grad)
    assert torch.equal(a(idx.int()), oa.detach())  # int32 indices
    # table-batched: [num_tables * B, L], table-major like the 1-D form
    tb = ops.TableBatchedTTEmbeddingBag(2, E_, D_, R, P, Q, use_cache=False, weight_dist="uniform", device="cpu", sparse=False)
    got = tb(idx)
    assert got.shape == (2, 3, D_) and torch.equal(got, tb(idx.reshape(-1), torch.arange(0, 31, 5)))
    with pytest.raises(ValueError):
        tb(idx[:5])  # 5 bags for 2 tables


def padded_batches():
    """(name, indices, offsets or None): padding at the front, in the middle and at the end of bags, an all-padding bag, a
    bag without padding, an empty 1-D bag"""
    x = PAD
    two_d = np.array([[x, 3, 9, 44, 12],      # front
                      [7, x, x, 100, 8],      # middle
                      [600, 2, 17, x, x],     # end
                      [x, x, x, x, x],        # all padding
                      [1, 2, 3, 4, 692],      # none
                      [x, 50, x, 51, x]], np.int64)
    one_d = np.array([x, 3, 9, 7, x, 100, x, x, 1, 2, 3, 600, x], np.int64)
    off = np.array([0, 3, 6, 6, 8, 11, 13], np.int64)  # bag 2 is empty, bag 3 all padding
    return [("2-D", two_d, None), ("1-D", one_d, off)]


@pytest.mark.parametrize("case", padded_batches(), ids=lambda c: c[0])
@pytest.mark.parametrize("ilo", [True, False], ids=["closing-offset", "bag-starts"])
def test_padded_sum_matches_torch_embedding_bag(ops, case, ilo):
    _, idx, off = case
    m = single(ops, padding_idx=PAD, include_last_offset=ilo)
    w = m.full_weight().detach().clone().requires_grad_(True)
    tidx = torch.from_numpy(idx)
    if off is None:
        out = m(tidx)
        ref = F.embedding_bag(tidx, w, None, mode="sum", padding_idx=PAD)
    else:
        toff = torch.from_numpy(off)
        out = m(tidx, toff if ilo else toff[:-1])
        ref = F.embedding_bag(tidx, w, toff, mode="sum", padding_idx=PAD, include_last_offset=True)
    assert_close(out.detach().numpy(), ref.detach().numpy(), "padded sum forward")
    allpad = 3
    assert (out.detach().numpy()[allpad] == 0).all(), "a bag of padding only is zero"
    d = torch.from_numpy(np.random.RandomState(2).standard_normal(tuple(out.shape)).astype(np.float32))
    out.backward(d)
    # the dense core gradients: those of the same bags without their padding slots, through torch's embedding_bag on the table
    keep = idx.reshape(-1) != PAD
    o = np.arange(0, idx.size + 1, idx.shape[1]) if off is None else off
    before = np.concatenate([[0], np.cumsum(keep)])
    plain = twin(ops, m, include_last_offset=True)
    po = plain(torch.from_numpy(idx.reshape(-1)[keep]), torch.from_numpy(before[o]))
    assert_close(po.detach().numpy(), ref.detach().numpy(), "hand-compacted forward")
    po.backward(d)
    ref.backward(d)
    assert (w.grad[PAD] == 0).all(), "torch gives the padding row no gradient"
    for k in range(3):
        assert_close(m.tt_cores[k].grad.numpy(), plain.tt_cores[k].grad.numpy(), f"grad{k} vs the hand-compacted batch")
    # ... and against autograd through the expanded table itself
    leaves = [c.detach().clone().requires_grad_(True) for c in m.tt_cores]
    full = ops.tt_matrix_to_full(P, Q, [1] + R + [1], leaves, [1, 0, 2, 3])
    if off is None:
        F.embedding_bag(tidx, full, None, mode="sum", padding_idx=PAD).backward(d)
    else:
        F.embedding_bag(tidx, full, torch.from_numpy(off), mode="sum", padding_idx=PAD, include_last_offset=True).backward(d)
    for k in range(3):
        assert_close(m.tt_cores[k].grad.numpy(), leaves[k].grad.numpy(), f"grad{k} vs torch on the expanded table")


def test_fused_sgd_step_equals_the_step_on_the_hand_compacted_batch(ops):
    _, idx, _ = padded_batches()[0]
    a = single(ops, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=PAD)
    b = twin(ops, a, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR)
    d = torch.from_numpy(np.random.RandomState(4).standard_normal((6, D_)).astype(np.float32))
    keep = idx.reshape(-1) != PAD
    before = np.concatenate([[0], np.cumsum(keep)])
    oa = a(torch.from_numpy(idx))
    ob = b(torch.from_numpy(idx.reshape(-1)[keep]), torch.from_numpy(before[::5]))
    assert torch.equal(oa, ob)
    oa.backward(d)
    ob.backward(d)
    for k in range(3):
        assert torch.equal(a.tt_cores[k], b.tt_cores[k]), f"core {k} after one fused SGD step"


def test_call_form_errors(ops):
    m = single(ops, padding_idx=PAD)
    idx2 = torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError):
        m(idx2, torch.tensor([0, 3, 6, 9, 12]))   # 2-D with offsets (as torch)
    with pytest.raises(ValueError):
        m(idx2.reshape(-1))                        # 1-D without offsets
    with pytest.raises(ValueError):
        single(ops)(idx2.reshape(-1))
    with pytest.raises(ValueError):
        single(ops)(idx2, torch.tensor([0, 3, 6, 9, 12]))
    with pytest.raises(ValueError):
        F.embedding_bag(idx2, torch.zeros(5, 2), torch.tensor([0, 3, 6, 9]))
    with pytest.raises(ValueError):
        m(idx2, per_sample_weights=torch.ones(12))  # weights must have the shape of indices
    assert m.prefetch(idx2) is False and m.prefetch_many([(idx2, None)]) is False
    assert single(ops).prefetch(idx2) is False


def test_compaction_kernels_use_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed): a 1024-thread work-group leaves 128 registers per lane"""
    from test_kernel_resources import resources

    res = resources("ttx_pad.hip")
    names = [k for k in res if "pad_" in k]
    assert len(names) == 7, names  # one-launch, count and compact kernels for one and two slots per load; the offsets gather
    for k in names:
        assert res[k]["ScratchSize"] == 0 and res[k]["VGPRs"] <= 128, (k, res[k])
