"""GPU tests of the pooling modes, padding_idx and the 2-D input on the mixed-cardinality modules, and of the kernel that builds
their batches: `ttx_bags_merge` against numpy through the raw C ABI, `MixedTTEmbeddingBag` / `VarTableTTEmbeddingBag` against
torch's own embedding_bag(mode=, padding_idx=) on every table's expanded matrix (forward, dense core gradients, fused SGD /
Adagrad steps, per_sample_weights), capture and replay, the refusals under capture, and that the sentinel never reaches a lookup."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_inputs as G
from test_pooling_modes_gpu import t
from util import EPS, LR, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -1


# ------------------------------------------------------------------------------------------------- the kernel through the C ABI
def np_merge(tabs, B, sentinel=SENTINEL):
    """the contract of ttx_bags_merge in numpy: concatenate, shift, cast, rewrite.  tabs: dicts of numpy arrays idx (1-D or
    [B, L]), off (or None), w (or None), pad (or None)"""
    out_i, out_o, out_w, base = [], [], [], 0
    for tb in tabs:
        flat = tb["idx"].reshape(-1).astype(np.int64)
        nnz = flat.size
        starts = np.arange(B, dtype=np.int64) * tb["idx"].shape[1] if tb["off"] is None else tb["off"][:B].astype(np.int64)
        out_o.append(np.clip(starts, 0, nnz) + base)
        out_i.append(flat if tb["pad"] is None else np.where(flat == tb["pad"], sentinel, flat))
        out_w.append(np.ones(nnz, np.float32) if tb["w"] is None else tb["w"].reshape(-1))
        base += nnz
    out_o.append(np.array([base], np.int64))
    return np.concatenate(out_i), np.concatenate(out_o), np.concatenate(out_w)


def raw_merge(dev_tabs, B, ilo, weighted, padded, fill=-7, out_shift=0):
    """ttx_bags_merge through the raw C ABI into buffers full of `fill`: every element it owes must be overwritten.  dev_tabs:
    dicts of device tensors (views allowed).  out_shift = 1: out_indices starts 8 bytes past a 16-byte boundary."""
    import tt_embeddings as E

    lib = E.lib()
    n = len(dev_tabs)
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    a_idx, a_off, a_w = (vp * n)(), (vp * n)(), (vp * n)()
    a_nnz, a_L, a_pad = (i64 * n)(), (i64 * n)(), (i64 * n)()
    a_ib, a_ob, a_has = (i32 * n)(), (i32 * n)(), (ctypes.c_uint8 * n)()
    for k, tb in enumerate(dev_tabs):
        a_idx[k], a_nnz[k], a_ib[k] = tb["idx"].data_ptr(), tb["idx"].numel(), tb["idx"].element_size()
        a_ob[k] = 8
        if tb["off"] is None:
            a_L[k] = tb["idx"].size(1)
        else:
            a_off[k], a_ob[k] = tb["off"].data_ptr(), tb["off"].element_size()
        if tb["w"] is not None:
            a_w[k] = tb["w"].data_ptr()
        if tb["pad"] is not None:
            a_pad[k], a_has[k] = tb["pad"], 1
    N = sum(a_nnz)
    buf_i = torch.full((N + out_shift,), fill, dtype=torch.int64, device=DEV)
    out_i = buf_i[out_shift:]
    out_o = torch.full((n * B + 1,), fill, dtype=torch.int64, device=DEV)
    out_w = torch.full((N,), float(fill), dtype=torch.float32, device=DEV)
    rc = lib.ttx_bags_merge(n, B, int(ilo), a_idx, a_nnz, a_ib, a_off, a_ob, a_L, a_w if weighted else None,
                            a_pad if padded else None, a_has if padded else None, SENTINEL, out_i.data_ptr(), out_o.data_ptr(),
                            out_w.data_ptr() if weighted else None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    if out_shift:
        assert int(buf_i[0]) == fill, "the slot in front of out_indices was written"
    return out_i.cpu().numpy(), out_o.cpu().numpy(), out_w.cpu().numpy()


NNZ = [1000, 7, 0, 40001, 1]  # per-table slot counts: odd bases, an empty table


def merge_case(ntab, B, ilo, seed=0):
    """tables cycling through the slot counts above, the three bag forms (int64 offsets, int32 offsets, 2-D), int64 / int32
    indices, weights on every third table, padding on every other one -- table k's padding value is live in table k + 1"""
    rs = np.random.RandomState(seed + 1000 * ntab + B)
    tabs = []
    for k in range(ntab):
        form = k % 3
        pad = k % 7 + 1 if k % 2 == 0 else None
        if form == 2:    # 2-D: B bags of L slots
            L = [0, 1, 7][(k // 3) % 3] if B > 5 else [0, 1, 7, 200][(k // 3) % 4]
            idx, off = rs.randint(0, 50, size=(B, L)), None
        else:
            nnz = NNZ[k % len(NNZ)]
            idx = rs.randint(0, 50, size=nnz)
            off = np.sort(rs.randint(0, nnz + 1, size=B + (1 if ilo else 0)))
            if ilo:
                off[-1] = nnz
            if k % 5 == 3 and B > 1:
                off[0], off[1] = -3, nnz + 9  # (clamped to [0, nnz])
            off = off.astype(np.int32 if form == 1 else np.int64)
        if idx.size and k > 0 and tabs[-1]["pad"] is not None:
            idx.reshape(-1)[0] = tabs[-1]["pad"]  # the neighbour's padding value: live here
        idx = idx.astype(np.int32 if k % 4 == 1 else np.int64)
        w = rs.standard_normal(idx.shape).astype(np.float32) if k % 3 == 0 else None
        tabs.append(dict(idx=idx, off=off, w=w, pad=pad))
    return tabs


def to_dev(tabs):
    return [dict(idx=t(tb["idx"]), off=None if tb["off"] is None else t(tb["off"]), w=None if tb["w"] is None else t(tb["w"]),
                 pad=tb["pad"]) for tb in tabs]


@pytest.mark.parametrize("B", [1, 5, 512])
@pytest.mark.parametrize("ntab", [1, 2, 3, 26, 64, 65])
def test_merge_kernel_vs_numpy(ntab, B):
    ilo = (ntab + B) % 2 == 0
    tabs = merge_case(ntab, B, ilo)
    ref_i, ref_o, ref_w = np_merge(tabs, B)
    dev = to_dev(tabs)
    out_i, out_o, out_w = raw_merge(dev, B, ilo, True, True)
    assert np.array_equal(out_o, ref_o), "out_offsets"
    assert np.array_equal(out_i, ref_i), "out_indices"
    assert np.array_equal(out_w, ref_w), "out_weights"
    again = raw_merge(dev, B, ilo, True, True, fill=-9)
    assert all(np.array_equal(a, b) for a, b in zip(again, (out_i, out_o, out_w))), "two runs, identical buffers"
    if ntab >= 3:
        bases = np.cumsum([0] + [tb["idx"].size for tb in tabs])
        assert (bases[1:ntab] % 2 == 1).any() and any(tb["idx"].size == 0 for tb in tabs), "an odd base and an empty table"
        # a padding value that is live in the next table survived there
        hit = [k for k in range(ntab - 1) if tabs[k]["pad"] is not None and tabs[k + 1]["idx"].size]
        assert hit and all(out_i[bases[k + 1]] == tabs[k]["pad"] for k in hit)
        assert (out_i == SENTINEL).any()
    # without weights / padding the arrays are not looked at and out_weights is not written
    plain_i, plain_o, plain_w = raw_merge(dev, B, ilo, False, False)
    assert np.array_equal(plain_o, ref_o) and (plain_w == -7).all()
    assert np.array_equal(plain_i, np.concatenate([tb["idx"].reshape(-1).astype(np.int64) for tb in tabs]))


def test_merge_kernel_on_pointers_aligned_to_their_element_only():
    """an int64 table that starts 8 bytes into an allocation, an int32 table that starts 4 bytes into one, behind a table of an odd
    number of slots, into an out_indices that starts 8 bytes past a 16-byte boundary"""
    rs = np.random.RandomState(3)
    B = 5
    tabs = []
    for k, (nnz, dt) in enumerate([(1001, np.int64), (2049, np.int64), (1500, np.int32), (3000, np.int64), (2, np.int64)]):
        off = np.sort(rs.randint(0, nnz + 1, size=B)).astype(np.int64)
        tabs.append(dict(idx=rs.randint(0, 30, size=nnz).astype(dt), off=off, w=None, pad=4 if k != 3 else None))
    dev = []
    for tb in tabs:
        buf = t(np.concatenate([[0], tb["idx"]]).astype(tb["idx"].dtype))
        dev.append(dict(idx=buf[1:], off=t(tb["off"]), w=None, pad=tb["pad"], keep=buf))
    assert dev[1]["idx"].data_ptr() % 16 == 8 and dev[2]["idx"].data_ptr() % 8 == 4
    ref_i, ref_o, _ = np_merge(tabs, B)
    for shift in (0, 1):
        out_i, out_o, _ = raw_merge(dev, B, False, False, True, out_shift=shift)
        assert np.array_equal(out_i, ref_i) and np.array_equal(out_o, ref_o), f"out_indices shifted by {shift}"


def test_bags_merge_is_merge_bags_for_int64_inputs_without_padding():
    import tt_embeddings as E
    import ttx_mixed

    rs = np.random.RandomState(4)
    for ilo in (False, True):
        idx, off = [], []
        for nnz in (1000, 0, 7, 40001):
            o = np.sort(rs.randint(0, nnz + 1, size=512 + (1 if ilo else 0)))
            o[0] = 0
            if ilo:
                o[-1] = nnz
            idx.append(t(rs.randint(0, 10 ** 7, size=nnz).astype(np.int64)))
            off.append(t(o.astype(np.int64)))
        mi, mo = ttx_mixed.merge_bags(idx, off, ilo)
        ki, ko, kw = E.bags_merge(idx, off, ilo)
        assert kw is None and ki.dtype == ko.dtype == torch.int64
        assert torch.equal(ki, mi) and torch.equal(ko, mo)
    # nothing to merge: the offsets owed are still written
    e = torch.empty(0, dtype=torch.int64, device=DEV)
    ki, ko, _ = E.bags_merge([e, e], [torch.zeros(3, dtype=torch.int64, device=DEV)] * 2, False)
    assert ki.numel() == 0 and ko.tolist() == [0] * 7
    ki, ko, _ = E.bags_merge([e], [e], False)
    assert ko.tolist() == [0]
    with pytest.raises(RuntimeError):
        E.bags_merge([e], [None], False)                      # 1-D without offsets
    with pytest.raises(RuntimeError):
        E.bags_merge([e.float()], [e], False)                 # dtype
    with pytest.raises(RuntimeError):
        E.bags_merge([e, e], [e, torch.zeros(1, dtype=torch.int64, device=DEV)], False)  # bag counts differ


# ------------------------------------------------------------------------------------------------------- modules against torch
# (name, cardinalities, p per table, q per table, ranks per table, constructor keywords)
GEOMS = [
    ("spec", [200, 700, 5000], [[5, 6, 7], [8, 9, 10], [20, 16, 16]], [[4, 4, 4]] * 3, [[32, 32]] * 3, {}),
    ("generic", [690, 120, 700], [[7, 9, 11], [4, 5, 6], [8, 9, 10]], [[3, 4, 5]] * 3, [[13, 12]] * 3, {}),
    ("table_q", [200, 700, 230], [[5, 6, 7], [8, 9, 10], [6, 5, 8]], [[4, 4, 4], [4, 4, 4], [2, 4, 8]],
     [[32, 32], [16, 16], [16, 16]], dict(pad_q=True, pad_ranks=True)),
]
GEOM_IDS = [g[0] for g in GEOMS]
PADS = [3, None, -1]
B_ = 5


def mixed(geom, mode, fused=True, padding_idx=PADS, **kw):
    """the module with "signed" cores (max meets no ties), and every table's cores in their natural shape"""
    import ttx_mixed

    _, Es, ps, qs, ranks, extra = geom
    D = int(np.prod(qs[0]))
    m = ttx_mixed.MixedTTEmbeddingBag(Es, D, ranks, ps, qs, weight_dist="uniform", device=DEV, fused=fused, mode=mode,
                                      padding_idx=padding_idx, **extra, **kw)
    for k in range(len(Es)):
        cores = G.make_cores(40 + k, 1, ps[k], qs[k], ranks[k], "signed")
        set_cores(m, k, [t(c[0]) for c in cores])
    return m


def where(m, k):
    g = next(i for i, tables in enumerate(m.group_tables) if k in tables)
    return m.groups[g], m.group_tables[g].index(k)


def natural(mod, j, arrays, t_):
    """table j's part of `arrays[t_]` (the cores or the optimizer state of a group module) in the table's own shape"""
    if not hasattr(mod, "table_rows"):
        return arrays[t_].detach()[j]
    rows = torch.split(arrays[t_].detach()[0], [p[t_] for p in mod.tt_p_shapes])[j]
    if mod.table_ranks is None and mod.table_q is None:
        return rows
    r0, q, r1 = mod._table_dims(j, t_)
    return rows.view(-1, mod.tt_ranks[t_], mod.tt_q_shapes[t_], mod.tt_ranks[t_ + 1])[:, :r0, :q, :r1].reshape(rows.size(0), -1)


def set_cores(m, k, cores):
    mod, j = where(m, k)
    with torch.no_grad():
        for t_, c in enumerate(cores):
            if hasattr(mod, "set_table_core"):
                mod.set_table_core(j, t_, c)
            else:
                mod.tt_cores[t_][j].copy_(c)


def get_cores(m, k):
    mod, j = where(m, k)
    return [natural(mod, j, list(mod.tt_cores), t_).clone() for t_ in range(3)]


def get_state(m, k):
    mod, j = where(m, k)
    return [natural(mod, j, list(mod.optimizer_state), t_).clone() for t_ in range(3)]


def get_grads(m, k):
    mod, j = where(m, k)
    return [natural(mod, j, [c.grad for c in mod.tt_cores], t_) for t_ in range(3)]


def batch(geom, seed, empty_table=1, all_padding_table=None, two_d=()):
    """per table (indices, offsets with the closing entry): B = 5 bags of 0..7 slots, bag 1 empty, bag 2 of padding only; one
    table without any lookup; every padding value live in the other tables; tables in `two_d` as [B, 4] with offsets None"""
    Es = geom[1]
    pads = [None if v is None else v % e for v, e in zip(PADS, Es)]
    rs = np.random.RandomState(seed)
    idx, off = [], []
    for k, e in enumerate(Es):
        lens = rs.randint(0, 8, size=B_)
        lens[1], lens[2] = 0, 3
        if k == empty_table:
            lens[:] = 0
        if k in two_d:
            lens[:] = 4
        o = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        i = rs.randint(0, e, size=int(o[-1])).astype(np.int64)
        mine = 3 if pads[k] is None else pads[k]
        i[rs.rand(i.size) < 0.3] = mine
        i[o[2]:o[3]] = mine
        if k == all_padding_table:
            i[:] = mine
        else:
            for j, other in enumerate(v for v in pads if v is not None and v != mine and v < e):
                if j < i.size and not o[2] <= j < o[3]:
                    i[j] = other
        idx.append(i.reshape(B_, 4) if k in two_d else i)
        off.append(None if k in two_d else o)
    return idx, off


def torch_reference(geom, k, cores, idx, off, mode, pad, d, weights=None):
    """F.embedding_bag on table k's expanded matrix -> (output, core gradients[, weight gradient])"""
    import tt_embeddings_ops as ops

    _, Es, ps, qs, ranks, _ = geom
    leaves = [c.detach().clone().requires_grad_(True) for c in cores]
    W = ops.tt_matrix_to_full(ps[k], qs[k], [1] + ranks[k] + [1], leaves, [1, 0, 2, 3])[:Es[k]]
    w = None if weights is None else weights.detach().clone().requires_grad_(True)
    if off is None:
        ref = F.embedding_bag(t(idx), W, None, mode=mode, padding_idx=pad, per_sample_weights=w)
    else:
        ref = F.embedding_bag(t(idx), W, t(off), mode=mode, padding_idx=pad, include_last_offset=True,
                              per_sample_weights=None if w is None else w.reshape(-1))
    ref.backward(d)
    return ref.detach(), [c.grad for c in leaves], None if w is None else w.grad


def call(m, idx, off, weights=None):
    return m([t(i) for i in idx], [None if o is None else t(o) for o in off], weights)


def grads_out(geom, seed):
    D = int(np.prod(geom[3][0]))
    return [t(G.make_grad(seed + k, 1, B_, D)[0]) for k in range(3)]


@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("geom,fused", [(g, True) for g in GEOMS] + [(GEOMS[0], False)], ids=GEOM_IDS + ["spec-grouped"])
def test_forward_and_dense_gradients_match_torch(geom, fused, mode):
    for two_d in ((), (0, 2)):
        m = mixed(geom, mode, fused=fused, sparse=False, include_last_offset=True)
        idx, off = batch(geom, 7, two_d=two_d)
        d = grads_out(geom, 70)
        outs = call(m, idx, off)
        sum((o * g).sum() for o, g in zip(outs, d)).backward()
        for k in range(3):
            pad = m.padding_idx[k]
            ref, grads, _ = torch_reference(geom, k, get_cores(m, k), idx[k], off[k], mode, pad, d[k])
            assert_close(outs[k].detach().cpu().numpy(), ref.cpu().numpy(), f"{mode} table {k} forward")
            if k == 1:
                assert (outs[k].detach() == 0).all(), "a table without lookups pools to zeros"
            if pad is not None and off[k] is not None:
                assert (outs[k].detach()[1:3] == 0).all(), "an empty bag and a bag of padding only are zero"
            for t_, g in enumerate(get_grads(m, k)):
                assert_close(g.cpu().numpy(), grads[t_].cpu().numpy(), f"{mode} table {k} grad{t_}")


@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_fused_optimizer_steps_track_torch_gradients(geom, mode, optim):
    """three fused steps on changing batches: after each, every table's cores (and Adagrad's state) are the update of the cores
    before the step along torch's gradient at those cores; zero-padded ranks / factorings stay zero"""
    import tt_embeddings_ops as ops

    opt = ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD
    m = mixed(geom, mode, sparse=True, optimizer=opt, learning_rate=LR, eps=EPS, include_last_offset=True)
    for step in range(3):
        idx, off = batch(geom, 80 + step, empty_table=step, two_d=(0,) if step == 1 else ())
        d = grads_out(geom, 90 + 3 * step)
        before = [get_cores(m, k) for k in range(3)]
        state0 = [get_state(m, k) for k in range(3)] if optim == "adagrad" else None
        outs = call(m, idx, off)
        sum((o * g).sum() for o, g in zip(outs, d)).backward()
        for k in range(3):
            _, grads, _ = torch_reference(geom, k, before[k], idx[k], off[k], mode, m.padding_idx[k], d[k])
            after = get_cores(m, k)
            for t_ in range(3):
                g, w0, got = grads[t_].cpu().numpy(), before[k][t_].cpu().numpy(), after[t_].cpu().numpy()
                if optim == "sgd":
                    assert_close(got, w0 - np.float32(LR) * g, f"step {step} sgd table {k} core{t_}")
                else:
                    s0 = state0[k][t_].cpu().numpy()
                    s = s0 + g * g
                    assert_close(get_state(m, k)[t_].cpu().numpy(), s, f"step {step} adagrad table {k} state{t_}")
                    assert_adagrad_close(got, w0 - np.float32(LR) * g / (np.sqrt(s) + np.float32(EPS)), g,
                                         f"step {step} adagrad table {k} core{t_}", state0=s0)
    mod = m.groups[0]
    if mod.table_ranks is not None or mod.table_q is not None:
        for k in range(3):
            for t_ in range(3):
                stored = mod.table_rows(t_)[k].clone()
                mod.set_table_core(k, t_, mod.table_core(k, t_).clone())  # (natural shape back in: the padding rewritten as zeros)
                assert torch.equal(mod.table_rows(t_)[k], stored), f"table {k} core {t_}: the padding did not stay zero"


def test_weighted_sum_with_padding_matches_torch():
    geom = GEOMS[0]
    m = mixed(geom, "sum", sparse=False, include_last_offset=True)
    idx, off = batch(geom, 101, empty_table=None, two_d=(2,))
    d = grads_out(geom, 102)
    rs = np.random.RandomState(103)
    ws = [t(rs.standard_normal(idx[0].shape).astype(np.float32)).requires_grad_(True), None,
          t(rs.standard_normal(idx[2].shape).astype(np.float32)).requires_grad_(True)]
    outs = call(m, idx, off, ws)
    sum((o * g).sum() for o, g in zip(outs, d)).backward()
    for k in range(3):
        pad = m.padding_idx[k]
        ref, grads, wgrad = torch_reference(geom, k, get_cores(m, k), idx[k], off[k], "sum", pad, d[k], weights=ws[k])
        assert_close(outs[k].detach().cpu().numpy(), ref.cpu().numpy(), f"weighted table {k} forward")
        for t_, g in enumerate(get_grads(m, k)):
            assert_close(g.cpu().numpy(), grads[t_].cpu().numpy(), f"weighted table {k} grad{t_}")
        if ws[k] is not None:
            got = ws[k].grad.cpu().numpy()
            assert got.shape == idx[k].shape
            assert_close(got, wgrad.cpu().numpy(), f"table {k} weight gradient")
            assert (got[idx[k] == pad] == 0).all() and (idx[k] == pad).any(), "padding slots get a zero weight gradient"
            assert np.abs(got[idx[k] != pad]).min() > 0


# ------------------------------------------------------------------------------------------------------------------ capture
def padded_2d(seed, Es, L, fill, pad):
    """per table [B, L] int64, every slot live with probability `fill`"""
    rs = np.random.RandomState(seed)
    out = []
    for e in Es:
        i = rs.randint(0, e, size=(64, L)).astype(np.int64)
        i[i == pad] = pad + 1
        i[rs.rand(64, L) >= fill] = pad
        out.append(i)
    return out


@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_captured_padded_step_replays_bit_identically_to_eager_steps(mode):
    """one fused group, padding_idx and 2-D inputs: the merge, the compaction, the lookup and the fused SGD step in ONE graph
    on one stream; three batches (one of them all padding) copied into the static tensors between replays"""
    import tt_embeddings_ops as ops
    import ttx_graph

    geom = ("cap", [3000, 9000, 11 * 10 ** 6], [[12, 16, 16], [20, 22, 25], [200, 220, 250]], [[4, 4, 4]] * 3, [[32, 32]] * 3, {})
    Es, pad, L = geom[1], 3, 12
    example = padded_2d(110, Es, L, 0.5, pad)
    patterns = [padded_2d(111, Es, L, 0.2, pad), [np.full((64, L), pad, np.int64)] * 3, padded_2d(112, Es, L, 0.9, pad)]
    g = t(G.make_grad(113, 3, 64, 64))
    outs = {False: [], True: []}

    def run(graphed):
        m = mixed(geom, mode, padding_idx=pad, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR)
        assert len(m.groups) == 1 and m.groups[0].padding_idx == SENTINEL
        seen = torch.zeros(3, 64, 64, device=DEV)

        def step(i0, i1, i2, d):
            res = m([i0, i1, i2], [None, None, None])
            out = torch.stack(res)
            seen.copy_(out.detach())
            out.backward(d)

        if graphed:
            gs = ttx_graph.GraphedStep(step, [t(i) for i in example] + [g], warmup=2)
        else:
            for _ in range(2):
                step(*[t(i) for i in example], g)
        for pat in patterns:
            if graphed:
                gs(*[t(i) for i in pat], g)
            else:
                step(*[t(i) for i in pat], g)
            torch.cuda.synchronize()
            outs[graphed].append(seen.clone())
        return [c.detach().clone() for c in m.groups[0].tt_cores]

    eager, replayed = run(False), run(True)
    for k in range(3):
        assert torch.equal(eager[k], replayed[k]), f"{mode}: core {k} differs between replay and eager"
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b), f"{mode}: output differs between replay and eager"
    assert (outs[True][1] == 0).all(), "the all-padding batch pools to zeros"
    assert outs[True][0].abs().max() > 0 and outs[True][2].abs().max() > 0


def test_var_table_module_takes_the_keywords_and_the_2d_form():
    """VarTableTTEmbeddingBag itself: one padding value for all tables, [num_tables * B, L] in, bit-identical to the 1-D call"""
    import tt_embeddings_ops as ops
    import ttx_mixed

    Es, ps = [200, 700, 5000], [[5, 6, 7], [8, 9, 10], [20, 16, 16]]
    idx2 = np.concatenate(padded_2d(120, Es, 6, 0.6, 3))
    res, first = [], None
    for two_d in (True, False):
        m = ttx_mixed.VarTableTTEmbeddingBag(Es, 64, [32, 32], ps, [4, 4, 4], sparse=True, optimizer=ops.OptimType.SGD,
                                             learning_rate=LR, weight_dist="uniform", device=DEV, mode="mean", padding_idx=-197)
        assert m.padding_idx == 3
        if first is None:
            first = [c.detach().clone() for c in m.tt_cores]
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, first):
                dst.copy_(src)
        out = m(t(idx2)) if two_d else m(t(idx2.reshape(-1)), torch.arange(0, idx2.size + 1, 6, device=DEV))
        assert out.shape == (3, 64, 64)
        out.backward(t(G.make_grad(121, 3, 64, 64)))
        res.append([out.detach().clone()] + [c.detach().clone() for c in m.tt_cores])
    assert all(torch.equal(a, b) for a, b in zip(*res))
    assert res[0][0].abs().max() > 0 and not torch.equal(res[0][1], first[0])


def test_refusals_under_capture_are_the_parents(monkeypatch):
    geom = GEOMS[0]
    idx, off = batch(geom, 130)
    mx = mixed(geom, "max", sparse=False, include_last_offset=True)
    ms = mixed(geom, "sum", sparse=False, include_last_offset=True)
    ws = [torch.ones(idx[0].size, device=DEV), None, None]
    with monkeypatch.context() as mp:  # (as if a capture were under way: nothing is captured, nothing left behind on the device)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="mode='max' reads the live count back"):
            call(mx, idx, off)
        with pytest.raises(RuntimeError, match="per_sample_weights drops the padding with torch ops"):
            call(ms, idx, off, ws)
    assert call(mx, idx, off)[0].shape == (B_, 64)  # (eagerly both are served)
    assert call(ms, idx, off, ws)[0].shape == (B_, 64)
    with pytest.raises(ValueError):
        call(mixed(geom, "mean", include_last_offset=True), idx, off, ws)


# -------------------------------------------------------------------------------------------- the sentinel reaches no lookup
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
def test_an_all_padding_table_is_zero_and_keeps_its_cores(mode):
    import tt_embeddings_ops as ops

    geom = GEOMS[0]
    m = mixed(geom, mode, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, include_last_offset=True)
    idx, off = batch(geom, 140, empty_table=None, all_padding_table=2)
    assert idx[2].size > 0 and (idx[2] == geom[1][2] - 1).all()
    before = [get_cores(m, k) for k in range(3)]
    outs = call(m, idx, off)
    sum((o * g).sum() for o, g in zip(outs, grads_out(geom, 141))).backward()
    torch.cuda.synchronize()
    assert (outs[2].detach() == 0).all()
    assert all(torch.equal(a, b) for a, b in zip(before[2], get_cores(m, 2))), "no row of the all-padding table was trained"
    assert any(not torch.equal(a, b) for a, b in zip(before[0], get_cores(m, 0)))
