"""CPU tests (no GPU) of the pooling modes, padding_idx and the 2-D input on the mixed-cardinality modules
(`MixedTTEmbeddingBag`, `VarTableTTEmbeddingBag`): the keywords' validation, the modules against torch's own
embedding_bag(mode=, padding_idx=) on every table's expanded matrix, the default call form, and the compiler's resource report of
the merge kernel.  The modules run on the oracle engine; what it lacks -- tables of different row factors in one lookup, the
pooling modes' entry points -- is stated below in plain torch (float64), for this file only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle_engine
from util import assert_close

D_, Q_, R_ = 12, [2, 3, 2], [4, 5]
ES = [100, 700, 90]                          # tables 0 and 2 share their row factors (one group when fused=False), not their size
PS = [[4, 5, 5], [8, 9, 10], [4, 5, 5]]
PADS = [3, None, -1]                         # per table: a value, none, the last row
B_ = 6


# ------------------------------------------------------------------------------------------------ the engine under the modules
def _per_table(p):
    return len(p) > 0 and isinstance(p[0], (list, tuple))


def _rows(p, q, r, cores, indices, tableidx):
    """[nnz, D] float64, differentiable in `cores`: row indices[n] of table tableidx[n].  p: one list (cores [tables, p_t, slice])
    or one list per table (cores [1, sum_k p_k_t, slice])"""
    T = len(q)
    tables = p if _per_table(p) else [list(p)] * int(cores[0].size(0))
    n = indices.numel()
    tb = tableidx.long()
    pt = torch.tensor(tables, dtype=torch.int64)                                       # [tables, T]
    base = torch.cat([torch.zeros(1, T, dtype=torch.int64), torch.cumsum(pt, 0)[:-1]])  # first slice of table k in core t
    rest, digits = indices.long(), [None] * T
    for s in reversed(range(T)):
        digits[s] = rest % pt[tb, s]
        rest = rest // pt[tb, s]
    flat = [c.reshape(-1, c.size(-1)).double() for c in cores]
    acc = flat[0][base[tb, 0] + digits[0]].reshape(n, q[0], r[1])
    for s in range(1, T):
        acc = torch.bmm(acc, flat[s][base[tb, s] + digits[s]].reshape(n, r[s], q[s] * r[s + 1])).reshape(n, -1, r[s + 1])
    return acc.reshape(n, -1)


def _core_grads(p, q, r, cores, indices, tableidx, d_rows):
    leaves = [c.detach().clone().requires_grad_(True) for c in cores]
    if indices.numel() == 0:
        return [torch.zeros_like(c) for c in leaves]
    with torch.enable_grad():  # (called from inside an autograd node's backward)
        _rows(p, q, r, leaves, indices, tableidx).backward(d_rows.double())
    return [c.grad for c in leaves]


class Engine:
    """oracle_engine, plus tables of different row factors and the pooling modes' entry points"""
    OPTIM_SGD, OPTIM_ADAGRAD, OPTIM_DENSE = 0, 1, 2

    def __getattr__(self, name):
        return getattr(oracle_engine, name)

    def make_plan(self, *a, **kw):
        return None

    def tt_forward(self, batch_count, num_tables, B, D, p, q, r, L, nnz, indices, rowidx, tableidx, tt_cores):
        if not _per_table(p):
            return oracle_engine.tt_forward(batch_count, num_tables, B, D, p, q, r, L, nnz, indices, rowidx, tableidx, tt_cores)
        out = torch.zeros(num_tables * B, D, dtype=torch.float64)
        if nnz:
            out.index_add_(0, tableidx * B + rowidx, _rows(p, q, r, [c.detach() for c in tt_cores], indices, tableidx))
        return out.float().view(num_tables, B, D)

    def tt_dense_backward(self, batch_count, D, p, q, r, L, nnz, indices, rowidx, tableidx, d_output, tt_cores):
        if not _per_table(p):
            return oracle_engine.tt_dense_backward(batch_count, D, p, q, r, L, nnz, indices, rowidx, tableidx, d_output, tt_cores)
        B = d_output.size(1)
        return _core_grads(p, q, r, tt_cores, indices, tableidx, d_output.reshape(-1, D)[tableidx * B + rowidx])

    def bag_mean_scale(self, x, offsets):
        n = (offsets[1:] - offsets[:-1]).clamp(min=1).to(x.dtype)
        return (x.reshape(-1, x.size(-1)) / n[:, None]).view_as(x)

    def tt_rows_p(self, num_tables, D, p, q, r, indices, tableidx, tt_cores, plan=None):
        if indices.numel() == 0:
            return torch.zeros(0, D)
        return _rows(p, q, r, [c.detach() for c in tt_cores], indices, tableidx).float()

    def bag_max_pool(self, rows, offsets):
        nb, D = offsets.numel() - 1, rows.size(1)
        out, arg = torch.zeros(nb, D), torch.full((nb, D), -1, dtype=torch.int32)
        for b in range(nb):
            s, e = int(offsets[b]), int(offsets[b + 1])
            if e > s:
                out[b], a = rows[s:e].max(0)
                arg[b] = (a + s).int()
        return out, arg

    def bag_max_pool_backward(self, d_output, argmax, offsets, nnz):
        D = argmax.size(-1)
        d_rows = torch.zeros(nnz, D)
        d, a = d_output.reshape(-1, D), argmax.reshape(-1, D).long()
        hit = a >= 0
        cols = torch.arange(D).expand_as(a)
        d_rows[a[hit], cols[hit]] = d[hit]
        return d_rows

    def tt_backward_rows(self, optim, D, lr, eps, p, q, r, nnz, indices, tableidx, d_rows, tt_cores, state=None, plan=None):
        assert optim == self.OPTIM_DENSE, "this file checks the dense gradients"
        return [g.float() for g in _core_grads(p, q, r, tt_cores, indices, tableidx, d_rows)]


@pytest.fixture()
def ops(monkeypatch):
    import tt_embeddings_ops as m

    monkeypatch.setattr(m, "_engine", Engine())
    return m


def mixed(**kw):
    import ttx_mixed

    torch.manual_seed(5)
    kw.setdefault("sparse", False)
    return ttx_mixed.MixedTTEmbeddingBag(ES, D_, R_, PS, Q_, weight_dist="uniform", device="cpu", **kw)


# ------------------------------------------------------------------------------------------------------------------ validation
def test_mixed_keywords_are_validated(ops):
    assert mixed().padding_idx == [None, None, None] and mixed().mode == "sum"
    assert mixed(padding_idx=None).padding_idx == [None, None, None]
    assert mixed(padding_idx=7).padding_idx == [7, 7, 7]
    assert mixed(padding_idx=-1).padding_idx == [99, 699, 89], "every value against its own table's cardinality"
    assert mixed(padding_idx=PADS).padding_idx == [3, None, 89]
    assert mixed(padding_idx=(np.int64(5), -700, None)).padding_idx == [5, 0, None]
    for fused in (False, True):
        m = mixed(fused=fused, mode="max", padding_idx=PADS)
        assert all(g.mode == "max" for g in m.groups)
        padded = [any(PADS[k] is not None for k in tables) for tables in m.group_tables]
        assert [g.padding_idx for g in m.groups] == [-1 if x else None for x in padded], "the groups compact on the sentinel"
    for bad in ("avg", None, "SUM"):
        with pytest.raises(ValueError):
            mixed(mode=bad)
    for bad in ([1, 2], [1, 2, 3, 4], 90, [0, 0, 90], [0, 700, 0], -101, [None, None, -91], 1.5, [True, None, None], "3"):
        with pytest.raises(ValueError):
            mixed(padding_idx=bad)


def test_var_table_keywords_are_validated(ops):
    import ttx_mixed

    def var(**kw):
        return ttx_mixed.VarTableTTEmbeddingBag(ES, D_, R_, PS, Q_, weight_dist="uniform", device="cpu", **kw)

    assert var().mode == "sum" and var().padding_idx is None
    assert var(mode="mean", padding_idx=89).padding_idx == 89
    assert var(padding_idx=-1).padding_idx == 89, "torch's rule against the smallest table"
    for bad in (90, 99, 699, -91):  # rows of the larger tables only
        with pytest.raises(ValueError):
            var(padding_idx=bad)
    with pytest.raises(ValueError):
        var(mode="avg")
    assert list(var(mode="max", padding_idx=3).state_dict()) == list(var().state_dict())
    # max on per-table row factors: three cores; the two- and four-core geometry classes are refused by name
    for ps, q, r in (([[5, 8], [6, 7]], [3, 4], [6]), ([[4, 5, 3, 4], [3, 4, 5, 2]], [2, 2, 2, 2], [3, 3, 3])):
        Es = [int(np.prod(p)) for p in ps]
        for mode in ("sum", "mean"):
            ttx_mixed.VarTableTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, weight_dist="uniform", device="cpu", mode=mode)
        with pytest.raises(NotImplementedError, match="three TT cores"):
            ttx_mixed.VarTableTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, weight_dist="uniform", device="cpu", mode="max")
        with pytest.raises(NotImplementedError, match="three TT cores"):
            ttx_mixed.MixedTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, weight_dist="uniform", device="cpu", mode="max", fused=True)


# ---------------------------------------------------------------------------------------------------------- against torch
def batch(seed, two_d=()):
    """per table (indices, offsets): bags of 0..5 slots, bag 1 empty, bag 2 of padding only (of the table's own padding value, or
    of row 3), every padding value live in the other tables; tables in `two_d` come as [B, 4] with offsets None"""
    rs = np.random.RandomState(seed)
    pads = [None if v is None else v % e for v, e in zip(PADS, ES)]
    idx, off = [], []
    for k, e in enumerate(ES):
        lens = rs.randint(0, 6, size=B_)
        lens[1], lens[2] = 0, 3
        if k in two_d:
            lens[:] = 4
        o = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        i = rs.randint(0, e, size=int(o[-1])).astype(np.int64)
        mine = 3 if pads[k] is None else pads[k]
        i[rs.rand(i.size) < 0.3] = mine
        i[o[2]:o[3]] = mine
        for j, other in enumerate(v for v in pads if v is not None and v != mine):
            if j < i.size and not o[2] <= j < o[3]:
                i[j] = other  # (3 and 89 are rows of every table)
        if k in two_d:
            idx.append(torch.from_numpy(i.reshape(B_, 4)))
            off.append(None)
        else:
            idx.append(torch.from_numpy(i))
            off.append(torch.from_numpy(o))
    return idx, off


def table_cores(m, k):
    """table k's cores [p_t, slice] and where their gradient sits: (group module, core -> gradient rows of the table)"""
    g = next(i for i, tables in enumerate(m.group_tables) if k in tables)
    mod, j = m.groups[g], m.group_tables[g].index(k)
    if hasattr(mod, "table_core"):
        sizes = [[p[t] for p in mod.tt_p_shapes] for t in range(3)]
        return [mod.table_core(j, t) for t in range(3)], lambda t: torch.split(mod.tt_cores[t].grad[0], sizes[t])[j]
    return [mod.tt_cores[t].detach()[j] for t in range(3)], lambda t: mod.tt_cores[t].grad[j]


def torch_reference(ops, m, k, idx, off, mode, pad, d):
    """F.embedding_bag on table k's expanded matrix -> (output, core gradients)"""
    leaves = [c.detach().clone().requires_grad_(True) for c in table_cores(m, k)[0]]
    W = ops.tt_matrix_to_full(PS[k], Q_, [1] + R_ + [1], leaves, [1, 0, 2, 3])[:ES[k]]
    if off is None:
        ref = F.embedding_bag(idx, W, None, mode=mode, padding_idx=pad)
    else:
        ref = F.embedding_bag(idx, W, off, mode=mode, padding_idx=pad, include_last_offset=True)
    ref.backward(d)
    return ref.detach(), [c.grad for c in leaves]


@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("fused", [False, True], ids=["grouped", "fused"])
def test_mixed_modes_match_torch_embedding_bag(ops, fused, mode, padded):
    pads = PADS if padded else None
    for ilo, two_d in ((True, ()), (False, (1,))):
        m = mixed(fused=fused, mode=mode, padding_idx=pads, include_last_offset=ilo)
        assert m.group_tables == ([[0, 1, 2]] if fused else [[0, 2], [1]])
        idx, off = batch(11, two_d)
        outs = m(idx, [o if o is None or ilo else o[:-1] for o in off])
        d = [torch.from_numpy(np.random.RandomState(20 + k).standard_normal((B_, D_)).astype(np.float32)) for k in range(3)]
        sum((o * g).sum() for o, g in zip(outs, d)).backward()
        for k in range(3):
            pad = m.padding_idx[k]
            ref, grads = torch_reference(ops, m, k, idx[k], off[k], mode, pad, d[k])
            assert outs[k].shape == (B_, D_)
            assert_close(outs[k].detach().numpy(), ref.numpy(), f"{mode} table {k} forward")
            if off[k] is not None:
                assert (outs[k].detach()[1] == 0).all(), "an empty bag is zero"
            if pad is not None:
                assert (outs[k].detach()[2] == 0).all(), "a bag of padding only is zero"
            grad_of = table_cores(m, k)[1]
            for t in range(3):
                assert_close(grad_of(t).numpy(), grads[t].numpy(), f"{mode} table {k} grad{t}")


# ------------------------------------------------------------------------------------------------------------------ the default
@pytest.mark.parametrize("fused", [False, True], ids=["grouped", "fused"])
def test_module_without_the_keywords_is_the_merge_bags_call_bit_for_bit(ops, fused):
    """sum, 1-D, per-table offsets: what the module ran before it had the keywords -- merge_bags() into the group module"""
    import ttx_mixed

    idx, off = batch(12)
    off = [o[:-1] for o in off]
    for kw in ({}, {"mode": "sum", "padding_idx": None}, {"padding_idx": [None] * 3}):
        m = mixed(fused=fused, **kw)
        outs = m(idx, off)
        for mod, tables in zip(m.groups, m.group_tables):
            assert mod.padding_idx is None and mod.mode == "sum"
            mi, mo = ttx_mixed.merge_bags([idx[k] for k in tables], [off[k] for k in tables], False)
            res = mod(mi, mo)
            for j, k in enumerate(tables):
                assert torch.equal(outs[k], res[j]), f"table {k}"


def test_call_form_errors(ops):
    m = mixed(padding_idx=PADS)
    idx, off = batch(13)
    off = [o[:-1] for o in off]
    with pytest.raises(ValueError):
        m([idx[0].reshape(-1, 1)] + idx[1:], off)                       # 2-D with offsets
    with pytest.raises(ValueError):
        m(idx, [None] + off[1:])                                        # 1-D without offsets
    with pytest.raises(ValueError):
        m(idx, [off[0][:-1]] + off[1:])                                 # tables that disagree on the number of bags
    with pytest.raises(ValueError):
        mixed(mode="mean")(idx, off, [torch.ones(idx[0].numel()), None, None])  # weights: sum only, as in torch


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_bags_merge_is_declared_and_exported_and_checks_its_arguments():
    """bad arguments: -1 with a message before anything is launched (the pointers below are never dereferenced)"""
    import ctypes
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "ttx.h")).read(), flags=re.S)
    assert re.search(r"\bttx_bags_merge\s*\(", hdr), "ttx_bags_merge is not declared in include/ttx.h"
    tables = int(re.search(r"#define\s+TTX_MAX_TABLES_MIXED\s+(\d+)", hdr).group(1))
    assert tables == 64, "the tables of one launch: their arguments must fit the kernel-argument segment"
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    fake = 4096
    for so in ("libttx.so", "libttx_hooks.so"):
        lib = ctypes.CDLL(os.path.join(root, "fbtt-embedding_amd", so))
        lib.ttx_last_error.restype = ctypes.c_char_p
        f = lib.ttx_bags_merge
        f.argtypes = [i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]

        def call(ntab=2, B=4, idx=(fake, fake), nnz=(40, 8), ib=(8, 8), off=(None, fake), ob=(8, 8), L=(10, 0), w=None,
                 pad=None, has=None, out_i=fake, out_o=fake, out_w=None):
            n = len(nnz)
            arr = lambda ty, v: None if v is None else (ty * n)(*v)  # noqa: E731
            return f(ntab, B, 0, arr(vp, idx), arr(i64, nnz), arr(i32, ib), arr(vp, off), arr(i32, ob), arr(i64, L), arr(vp, w),
                     arr(i64, pad), arr(ctypes.c_uint8, has), -1, out_i, out_o, out_w, None)

        for what, kw in (("ntab < 1", dict(ntab=0)), ("negative B", dict(B=-1)), ("negative nnz", dict(nnz=(40, -8))),
                         ("N >= 2^31", dict(nnz=(1 << 30, 1 << 30), off=(fake, fake))), ("nnz != B L", dict(L=(9, 0))),
                         ("negative L", dict(nnz=(-40, 8), L=(-10, 0))), ("NULL indices", dict(idx=(None, fake))),
                         ("NULL per-table arrays", dict(idx=None)), ("NULL out_indices", dict(out_i=None)),
                         ("NULL out_offsets", dict(out_o=None)), ("NULL out_weights", dict(w=(fake, None))),
                         ("element width", dict(ib=(8, 2))), ("misaligned int64 indices", dict(idx=(fake + 4, fake))),
                         ("misaligned offsets", dict(off=(None, fake + 4))), ("padding without flags", dict(pad=(1, 2)))):
            assert call(**kw) == -1, what
            assert b"bags_merge" in lib.ttx_last_error(), (what, lib.ttx_last_error())


def test_engine_exposes_bags_merge():
    import tt_embeddings as E

    with pytest.raises(RuntimeError):  # (no CPU path in the engine: GPU tensors only)
        E.bags_merge([torch.zeros(4, dtype=torch.int64)], [torch.zeros(2, dtype=torch.int64)], False)
    with pytest.raises(RuntimeError):
        E.bags_merge([], [], False)


# ---------------------------------------------------------------------------------------------------------- compiler resources
def test_merge_kernel_uses_no_scratch():
    """the compiler's own resource report for gfx950 (no GPU needed): the per-table arguments are subscripted at run time and
    must still be read from the argument segment, not from a copy in scratch memory"""
    from test_kernel_resources import resources

    res = resources("ttx_merge.hip")
    assert res, "no kernel in ttx_merge.hip"
    assert not [k for k in res if "pad_" in k]
    for k, v in res.items():
        assert v["ScratchSize"] == 0, (k, v)
