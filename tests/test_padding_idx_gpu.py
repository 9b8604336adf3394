"""GPU tests of nn.EmbeddingBag's padded batches on the TT bags (`padding_idx`, the 2-D fixed-length input): the compaction
kernel against numpy through the C ABI, the module against torch's own embedding_bag(padding_idx=) on the looked-up rows of
the expanded table (forward, dense core gradients, fused SGD / Adagrad steps) in all three pooling modes, bit identity with
the hand-compacted forward(n_dev=) call, the frequency table, capture, per_sample_weights, the refusals and the default."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gen_inputs as G
from test_pooling_modes_gpu import GEOM_IDS, GEOMS, t, tt_rows_torch, use_route
from util import EPS, LR, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 3  # (a valid row of every geometry below)


# ------------------------------------------------------------------------------------------------------------- references
def np_compact(idx, off, L, pad):
    """(out_indices, out_offsets, n): the contract of ttx_bags_compact in numpy"""
    flat = idx.reshape(-1)
    keep = flat != pad
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    o = np.arange(0, flat.size + 1, L, dtype=np.int64) if off is None else off
    out = np.zeros(flat.size, np.int64)
    n = int(keep.sum())
    out[:n] = flat[keep]
    out_off = before[o].copy()
    out_off[-1] = n
    return out, out_off, n


def raw_compact(idx, off, L, pad, fill=-7):
    """ttx_bags_compact through the raw C ABI into buffers full of `fill`: every element it owes must be overwritten"""
    import tt_embeddings as E

    lib = E.lib()
    nnz = idx.numel()
    nb = off.numel() - 1 if off is not None else (nnz // L if L else 0)
    out_i = torch.full((nnz,), fill, dtype=torch.int64, device=DEV)
    out_o = torch.full((nb + 1,), fill, dtype=torch.int64, device=DEV)
    n_live = torch.full((1,), fill, dtype=torch.int32, device=DEV)
    nbytes = lib.ttx_bags_compact_workspace_bytes(nb, nnz)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
    rc = lib.ttx_bags_compact(nb, nnz, idx.data_ptr(), None if off is None else off.data_ptr(), L, pad, out_i.data_ptr(),
                              out_o.data_ptr(), n_live.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    return out_i.cpu().numpy(), out_o.cpu().numpy(), int(n_live.item())


def padded_2d(seed, N, L, E_, fill, pad=PAD):
    """[N, L] int64: every slot live with probability `fill` (padding anywhere in a bag), bag 0 all padding, bag 1 full"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, E_, size=(N, L)).astype(np.int64)
    idx[idx == pad] = pad + 1
    idx[rs.rand(N, L) >= fill] = pad
    if 0.0 < fill < 1.0 and N > 1:
        idx[0] = pad
        idx[1] = np.where(idx[1] == pad, pad + 1, idx[1])
    return idx


def padded_1d(seed, N, maxlen, E_, fill, pad=PAD):
    """ragged bags of 0..maxlen slots (bag 2 empty, bag 3 all padding) -> (indices, offsets with the closing entry)"""
    rs = np.random.RandomState(seed)
    lengths = rs.randint(0, maxlen + 1, size=N)
    if N > 3:
        lengths[2] = 0
        lengths[3] = max(1, lengths[3])
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = rs.randint(0, E_, size=int(off[-1])).astype(np.int64)
    idx[idx == pad] = pad + 1
    idx[rs.rand(idx.size) >= fill] = pad
    if N > 3:
        idx[off[3]:off[4]] = pad
    return idx, off


def ref_lookup_padded(p, q, ranks, cores, idx, off, num_tables, mode, pad=PAD, weights=None):
    """[num_tables, B, D] = torch's embedding_bag(mode=, padding_idx=) per table.  The table torch sees is the batch's own rows
    of the expanded table (tt_rows_torch: differentiable in the cores) plus one row that stands for `pad`: every slot looks up
    its own row, the padding slots that one."""
    flat = idx.reshape(-1)
    B = (off.size - 1) // num_tables
    outs = []
    for k in range(num_tables):
        o = off[k * B:(k + 1) * B + 1].astype(np.int64)
        s, e = int(o[0]), int(o[-1])
        rows = tt_rows_torch(p, q, ranks, [c[k] for c in cores], flat[s:e])
        table = torch.cat([rows, torch.zeros(1, rows.size(1), device=DEV)])
        pos = np.where(flat[s:e] == pad, e - s, np.arange(e - s)).astype(np.int64)
        w = None if weights is None else weights[s:e]
        outs.append(F.embedding_bag(t(pos), table, t(o - s), mode=mode, include_last_offset=True, padding_idx=e - s,
                                    per_sample_weights=w))
    return torch.stack(outs)


def module(p, q, r, cores, num_tables, mode, **kw):
    import tt_embeddings_ops as ops

    kw.setdefault("use_cache", False)
    m = ops.TableBatchedTTEmbeddingBag(num_tables, int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform",
                                       device=DEV, mode=mode, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(t(src))
    return m


# ------------------------------------------------------------------------------------------------- the kernel through the C ABI
# one launch up to 32,768 slots (cfg2 at 50 % fill: 512 x 40 = 20,480), tiles above; 16384 x 40 = 327,680 x 2 slots
SIZES_2D = [(1, 1), (4, 10), (3, 43), (512, 40), (1024, 32), (1025, 32), (2100, 16), (16384, 40)]


@pytest.mark.parametrize("fill", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N,L", SIZES_2D, ids=[f"{n}x{l}" for n, l in SIZES_2D])
def test_compact_kernel_2d_form_vs_numpy(N, L, fill):
    idx = padded_2d(N * 131 + L, N, L, 10 ** 7, fill)
    ref_i, ref_o, n = np_compact(idx, None, L, PAD)
    dev = t(idx.reshape(-1))
    out_i, out_o, n_live = raw_compact(dev, None, L, PAD)
    assert n_live == n == ref_o[-1] == out_o[-1]
    assert np.array_equal(out_o, ref_o), "out_offsets: live slots in front of every bag"
    assert np.array_equal(out_i[:n], ref_i[:n]), "the live slots, in their original order"
    assert (out_i[n:] == 0).all(), "the zero tail"
    again = raw_compact(dev, None, L, PAD, fill=-9)
    assert np.array_equal(again[0], out_i) and np.array_equal(again[1], out_o) and again[2] == n, "two runs, identical buffers"
    if fill == 0.0:
        assert n == 0 and (out_o == 0).all()
    if fill == 1.0:
        assert n == N * L and np.array_equal(out_i, idx.reshape(-1))


SIZES_1D = [(5, 4), (40, 300), (1024, 63), (1200, 64), (40000, 1), (16384, 80)]


@pytest.mark.parametrize("fill", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("N,maxlen", SIZES_1D, ids=[f"{n}bags-{l}" for n, l in SIZES_1D])
def test_compact_kernel_offsets_form_vs_numpy(N, maxlen, fill):
    idx, off = padded_1d(N * 17 + maxlen, N, maxlen, 10 ** 7, fill)
    ref_i, ref_o, n = np_compact(idx, off, 0, PAD)
    out_i, out_o, n_live = raw_compact(t(idx), t(off), 0, PAD)
    assert n_live == n == out_o[-1]
    assert np.array_equal(out_o, ref_o)
    assert np.array_equal(out_i[:n], ref_i[:n]) and (out_i[n:] == 0).all()
    assert (np.diff(out_o)[np.diff(off) == 0] == 0).all(), "empty bags give equal consecutive offsets"
    again = raw_compact(t(idx), t(off), 0, PAD, fill=-9)
    assert np.array_equal(again[0], out_i) and np.array_equal(again[1], out_o) and again[2] == n


@pytest.mark.parametrize("nnz", [1000, 20480, 70001])
def test_compact_kernel_on_an_8_byte_aligned_buffer_and_through_the_engine(nnz):
    """indices that start 8 bytes into an allocation take the one-slot-per-load kernels; the engine call allocates its outputs"""
    import tt_embeddings as E

    rs = np.random.RandomState(nnz)
    idx = rs.randint(0, 50, size=nnz + 1).astype(np.int64)  # (a small key space: about 2 % of the slots hold PAD)
    buf = t(idx)
    view = buf[1:]
    assert view.data_ptr() % 16 == 8
    off = np.array([0, 1, 1, nnz // 2, nnz], np.int64)
    ref_i, ref_o, n = np_compact(idx[1:], off, 0, PAD)
    out_i, out_o, n_live = raw_compact(view, t(off), 0, PAD)
    assert n_live == n and np.array_equal(out_o, ref_o) and np.array_equal(out_i, ref_i)
    e_i, e_o, e_n = E.bags_compact(view, t(off), 0, PAD)
    assert e_n.dtype == torch.int32 and int(e_n.item()) == n
    assert np.array_equal(e_i.cpu().numpy(), ref_i) and np.array_equal(e_o.cpu().numpy(), ref_o)
    z_i, z_o, z_n = E.bags_compact(torch.empty(0, dtype=torch.int64, device=DEV), torch.zeros(6, dtype=torch.int64, device=DEV), 0, PAD)
    assert z_i.numel() == 0 and (z_o == 0).all() and int(z_n.item()) == 0  # (nothing to compact: zeros, no launch)


# ------------------------------------------------------------------------------------------------------ module: the two call forms
MODE_ROUTES = [("sum", "native"), ("sum", "python"), ("mean", "native"), ("mean", "python"), ("max", "python")]
MODE_ROUTE_IDS = [f"{m}-{r}" for m, r in MODE_ROUTES]


def ref_grads(p, q, r, cores_np, idx, off, nt, mode, d_out, weights=None):
    leaves = [t(c).clone().requires_grad_(True) for c in cores_np]
    ref = ref_lookup_padded(p, q, r, leaves, idx, off, nt, mode, weights=weights)
    ref.backward(t(d_out))
    return ref.detach(), [c.grad.cpu().numpy() for c in leaves]


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("mode,route", MODE_ROUTES, ids=MODE_ROUTE_IDS)
def test_padded_forward_and_dense_gradients_match_torch(geom, mode, route, monkeypatch):
    """3 tables; the 2-D form (padding anywhere in a bag, an all-padding bag, a full bag) and 1-D indices + offsets (an empty
    bag too), with and without the closing offset"""
    use_route(route, monkeypatch)
    _, p, q, r = geom
    nt, B, L, E_, D = 3, 13, 9, int(np.prod(p)), int(np.prod(q))
    cores = G.make_cores(31, nt, p, q, r, "signed")
    d_out = G.make_grad(7, nt, B, D)
    # 2-D
    idx2 = padded_2d(5, nt * B, L, E_, 0.5)
    off2 = np.arange(0, idx2.size + 1, L, dtype=np.int64)
    ref, grads = ref_grads(p, q, r, cores, idx2, off2, nt, mode, d_out)
    m = module(p, q, r, cores, nt, mode, sparse=False, padding_idx=PAD)
    out = m(t(idx2))
    assert out.shape == (nt, B, D)
    assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), f"{mode} 2-D padded forward")
    assert (out.detach()[0, 0] == 0).all(), "a bag of padding only is zero"
    out.backward(t(d_out))
    for k in range(len(p)):
        assert_close(m.tt_cores[k].grad.cpu().numpy(), grads[k], f"{mode} 2-D padded grad{k}")
    # 1-D + offsets, both offset forms, int32, a negative padding_idx
    idx1, off1 = padded_1d(6, nt * B, 12, E_, 0.6)
    ref, grads = ref_grads(p, q, r, cores, idx1, off1, nt, mode, d_out)
    for ilo in (True, False):
        m1 = module(p, q, r, cores, nt, mode, sparse=False, padding_idx=PAD - E_, include_last_offset=ilo)
        out = m1(t(idx1).int(), t(off1 if ilo else off1[:-1]).int())
        assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), f"{mode} 1-D padded forward (closing offset: {ilo})")
        out.backward(t(d_out))
        for k in range(len(p)):
            assert_close(m1.tt_cores[k].grad.cpu().numpy(), grads[k], f"{mode} 1-D padded grad{k}")


@pytest.mark.parametrize("mode,route", MODE_ROUTES, ids=MODE_ROUTE_IDS)
def test_2d_input_without_padding_idx_is_the_flattened_1d_call(mode, route, monkeypatch):
    import tt_embeddings_ops as ops

    use_route(route, monkeypatch)
    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B, L = 2, 16, 7
    cores = G.make_cores(33, nt, p, q, r, "signed")
    idx = padded_2d(8, nt * B, L, int(np.prod(p)), 1.0)
    d = t(G.make_grad(9, nt, B, 64))
    res = []
    for two_d in (True, False):
        for ilo in (True, False):
            m = module(p, q, r, cores, nt, mode, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, include_last_offset=ilo)
            off = torch.arange(0, idx.size + 1, L, device=DEV)
            out = m(t(idx)) if two_d else m(t(idx.reshape(-1)), off if ilo else off[:-1])
            out.backward(d)
            res.append([out.detach().clone()] + [c.detach().clone() for c in m.tt_cores])
    for other in res[1:]:
        assert all(torch.equal(a, b) for a, b in zip(res[0], other))


# ----------------------------------------------------------------------------------------------------------- bit identity
@pytest.mark.parametrize("mode", ["sum", "mean"])
@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_padded_call_is_the_hand_compacted_n_dev_call_bit_for_bit(mode, optim):
    """the same capacity, the tail zeroed: the padded call IS forward(n_dev=) on the compacted buffer -- output, cores and
    optimizer state after a fused step.  (The exact-size 1-D call is compared at the default tolerance only: a plan built for a
    capacity larger than its live count may chunk differently.)"""
    import tt_embeddings_ops as ops

    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B, L, E_ = 2, 64, 12, int(np.prod(p))
    cores = G.make_cores(35, nt, p, q, r, "signed")
    idx = padded_2d(10, nt * B, L, E_, 0.5)
    comp, off, n = np_compact(idx, None, L, PAD)
    d = t(G.make_grad(11, nt, B, 64))
    kw = dict(sparse=True, optimizer=ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD, learning_rate=LR, eps=EPS)
    a = module(p, q, r, cores, nt, mode, padding_idx=PAD, **kw)
    b = module(p, q, r, cores, nt, mode, **kw)
    c = module(p, q, r, cores, nt, mode, **kw)
    oa = a(t(idx))
    ob = b(t(comp), t(off), n_dev=torch.tensor([n], dtype=torch.int32, device=DEV))
    oc = c(t(comp[:n]), t(off))
    assert torch.equal(oa, ob), "output"
    assert_close(oa.detach().cpu().numpy(), oc.detach().cpu().numpy(), "vs the exact-size call")
    oa.backward(d)
    ob.backward(d)
    for k in range(3):
        assert torch.equal(a.tt_cores[k], b.tt_cores[k]), f"core {k}"
        assert torch.equal(a.optimizer_state[k], b.optimizer_state[k]), f"state {k}"


# ------------------------------------------------------------------------------------------------------- fused optimizers
@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("mode", ["sum", "mean", "max"])
@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_fused_optimizer_steps_track_the_gradients(geom, mode, optim):
    """three fused steps on changing padded batches: after each, the cores (and Adagrad's state) are the update of the cores
    before the step along torch's gradient at those cores"""
    import tt_embeddings_ops as ops

    _, p, q, r = geom
    nt, B, L, E_, D = 2, 11, 10, int(np.prod(p)), int(np.prod(q))
    cores = G.make_cores(41, nt, p, q, r, "signed")
    opt = ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD
    m = module(p, q, r, cores, nt, mode, sparse=True, optimizer=opt, learning_rate=LR, eps=EPS, padding_idx=PAD)
    for step in range(3):
        idx = padded_2d(50 + step, nt * B, L, E_, 0.3 + 0.3 * step)
        off = np.arange(0, idx.size + 1, L, dtype=np.int64)
        d_out = G.make_grad(60 + step, nt, B, D)
        before = [c.detach().cpu().numpy().copy() for c in m.tt_cores]
        state0 = [s.cpu().numpy().copy() for s in m.optimizer_state] if optim == "adagrad" else None
        _, grads = ref_grads(p, q, r, before, idx, off, nt, mode, d_out)
        m(t(idx)).backward(t(d_out))
        for k in range(len(p)):
            got = m.tt_cores[k].detach().cpu().numpy()
            if optim == "sgd":
                assert_close(got, before[k] - np.float32(LR) * grads[k], f"step {step} sgd core{k}")
            else:
                s = state0[k] + grads[k] * grads[k]
                assert_close(m.optimizer_state[k].cpu().numpy(), s, f"step {step} adagrad state{k}")
                ref_w = before[k] - np.float32(LR) * grads[k] / (np.sqrt(s) + np.float32(EPS))
                assert_adagrad_close(got, ref_w, grads[k], f"step {step} adagrad core{k}", state0=state0[k])


# ------------------------------------------------------------------------------------------------------- frequency table
def test_padding_is_not_counted_by_the_frequency_table():
    """use_cache=True before cache_populate(): the table after a padded batch holds the keys and counts it holds after the
    compacted batch -- compared as (key, count) pairs, since concurrent inserts leave a key's SLOT to arrival order -- and
    padding_idx's row is not among them"""
    import tt_embeddings_ops as ops

    p, q, r = [20, 22, 25], [4, 4, 4], [16, 16]
    E_ = int(np.prod(p))
    rs = np.random.RandomState(70)
    keys = rs.choice(np.arange(10, E_), size=64, replace=False)
    idx = keys[rs.randint(0, 64, size=(32, 10))].astype(np.int64)
    idx[rs.rand(32, 10) < 0.5] = PAD
    comp, off, n = np_compact(idx, None, 10, PAD)
    tables = []
    for padded in (True, False):
        m = ops.TTEmbeddingBag(E_, 64, r, p, q, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, use_cache=True,
                               cache_size=32, hashtbl_size=1 << 16, weight_dist="uniform", device=DEV,
                               padding_idx=PAD if padded else None)
        with torch.no_grad():
            out = m(t(idx)) if padded else m(t(comp[:n]), t(off))
        assert out.shape == (32, 64)
        ht, cf = m.hashtbl.cpu().numpy(), m.cache_freq.cpu().numpy()
        assert (cf[ht < 0] == 0).all()
        tables.append(sorted((int(k), int(c)) for k, c in zip(ht[ht >= 0], cf[ht >= 0])))
    assert tables[0] == tables[1]
    want = {}
    for k in comp[:n]:
        want[int(k)] = want.get(int(k), 0) + 1
    assert tables[0] == sorted(want.items()), "every live lookup counted once"
    assert PAD not in dict(tables[0]), "padding_idx's row must not be counted"


# ------------------------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("mode", ["sum", "mean"])
def test_captured_padded_step_replays_bit_identically_to_eager_steps(mode):
    """one capture over a static [N, L] input; three padding patterns (one of them all padding) copied into it between replays"""
    import tt_embeddings_ops as ops
    import ttx_graph

    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B, L, E_ = 2, 64, 12, int(np.prod(p))
    cores = G.make_cores(101, nt, p, q, r, "signed")
    example = padded_2d(102, nt * B, L, E_, 0.5)
    patterns = [padded_2d(103, nt * B, L, E_, 0.2), np.full((nt * B, L), PAD, np.int64), padded_2d(104, nt * B, L, E_, 0.9)]
    g = t(G.make_grad(105, nt, B, 64))
    outs = {False: [], True: []}

    def run(graphed):
        m = module(p, q, r, cores, nt, mode, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=PAD)
        seen = torch.zeros(nt, B, 64, device=DEV)

        def step(i, d):
            out = m(i)
            seen.copy_(out.detach())
            out.backward(d)

        if graphed:
            gs = ttx_graph.GraphedStep(step, (t(example), g), warmup=2)
        else:
            for _ in range(2):
                step(t(example), g)
        for pat in patterns:
            if graphed:
                gs(t(pat), g)
            else:
                step(t(pat), g)
            torch.cuda.synchronize()
            outs[graphed].append(seen.clone())
        return [c.detach().clone() for c in m.tt_cores]

    eager, replayed = run(False), run(True)
    for k in range(3):
        assert torch.equal(eager[k], replayed[k]), f"{mode}: core {k} differs between replay and eager"
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b), f"{mode}: output differs between replay and eager"
    assert (outs[True][1] == 0).all(), "the all-padding batch pools to zeros"
    assert outs[True][0].abs().max() > 0 and outs[True][2].abs().max() > 0


# ----------------------------------------------------------------------------------------------------------- per_sample_weights
def test_weighted_sum_with_padding_matches_torch():
    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B, L, E_ = 2, 16, 9, int(np.prod(p))
    cores = G.make_cores(111, nt, p, q, r, "signed")
    idx = padded_2d(112, nt * B, L, E_, 0.5)
    off = np.arange(0, idx.size + 1, L, dtype=np.int64)
    w_np = np.random.RandomState(113).standard_normal(idx.shape).astype(np.float32)
    d_out = G.make_grad(114, nt, B, 64)
    w_ref = t(w_np.reshape(-1)).requires_grad_(True)
    ref, grads = ref_grads(p, q, r, cores, idx, off, nt, "sum", d_out, weights=w_ref)
    m = module(p, q, r, cores, nt, "sum", sparse=False, padding_idx=PAD)
    w = t(w_np).requires_grad_(True)
    out = m(t(idx), per_sample_weights=w)
    assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), "weighted padded forward")
    out.backward(t(d_out))
    for k in range(3):
        assert_close(m.tt_cores[k].grad.cpu().numpy(), grads[k], f"weighted padded grad{k}")
    assert w.grad.shape == w.shape
    assert_close(w.grad.cpu().numpy().reshape(-1), w_ref.grad.cpu().numpy(), "weight gradient")
    assert (w.grad.cpu().numpy()[idx == PAD] == 0).all(), "padding slots get a zero weight gradient"
    assert np.abs(w.grad.cpu().numpy()[idx != PAD]).min() > 0


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    cores = G.make_cores(121, 1, p, q, r, "signed")
    idx = t(padded_2d(122, 8, 6, int(np.prod(p)), 0.5))
    off = torch.arange(0, 49, 6, device=DEV)
    mx = module(p, q, r, cores, 1, "max", sparse=False, padding_idx=PAD)
    ms = module(p, q, r, cores, 1, "sum", sparse=False, padding_idx=PAD)
    plain = module(p, q, r, cores, 1, "sum", sparse=False)
    with monkeypatch.context() as mp:  # (as if a capture were under way: nothing is captured, nothing left behind on the device)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="mode='max' reads the live count back"):
            mx(idx)
        with pytest.raises(RuntimeError, match="per_sample_weights drops the padding with torch ops"):
            ms(idx, per_sample_weights=torch.ones(8, 6, device=DEV))
    assert mx(idx).shape == (1, 8, 64)  # (eagerly both are served)
    assert ms(idx, per_sample_weights=torch.ones(8, 6, device=DEV)).shape == (1, 8, 64)
    # nothing is planned ahead for a padded call
    assert ms.prefetch(idx.reshape(-1), off) is False and ms.prefetch(idx) is False
    assert ms.prefetch_many([(idx.reshape(-1), off)]) is False and plain.prefetch_many([(idx, None)]) is False
    assert plain.prefetch(idx) is False
    assert plain.prefetch(idx.reshape(-1), off) is True  # (the 1-D call of a module without padding_idx still is)
    with pytest.raises(ValueError):
        ms(idx, off)
    with pytest.raises(ValueError):
        ms(idx.reshape(-1))
    with pytest.raises(NotImplementedError):
        ms(idx, n_dev=torch.tensor([3], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        module(p, q, r, cores, 1, "mean", padding_idx=PAD)(idx, per_sample_weights=torch.ones(8, 6, device=DEV))


# --------------------------------------------------------------------------------------------------------------- the default
@pytest.mark.parametrize("route", ["native", "python"])
def test_padding_idx_none_is_the_default_bit_for_bit(route, monkeypatch):
    import tt_embeddings_ops as ops
    from test_pooling_modes_gpu import batch

    use_route(route, monkeypatch)
    p, q, r = [200, 220, 250], [4, 4, 4], [32, 32]
    nt, B = 2, 32
    cores = G.make_cores(131, nt, p, q, r, "signed")
    idx, off = batch(132, nt, B, int(np.prod(p)), long_bag=20)
    d = t(G.make_grad(133, nt, B, 64))
    res = []
    for kw in ({}, {"padding_idx": None}):
        m = ops.TableBatchedTTEmbeddingBag(nt, int(np.prod(p)), 64, r, p, q, use_cache=False, weight_dist="uniform", device=DEV,
                                           sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, **kw)
        with torch.no_grad():
            for dst, src in zip(m.tt_cores, cores):
                dst.copy_(t(src))
        out = m(t(idx), t(off))
        out.backward(d)
        res.append([out.detach().clone()] + [c.detach().clone() for c in m.tt_cores])
    assert all(torch.equal(a, b) for a, b in zip(*res))
