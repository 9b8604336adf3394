"""GPU tests of the unpooled lookup `TTEmbedding` (nn.Embedding on a TT table, with padding_idx): ttx_rows_expand /
ttx_rows_collect against numpy through the raw C ABI, the module against the float64 reference on every geometry (forward,
dense core gradients, fused SGD / Adagrad), the bit identities between its routes, the sizes that switch routes, capture with
a changing padding count, determinism and the refusals."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import tt_ref64 as R64
from test_pooling_modes_gpu import GEOMS, t
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 5
# ... plus a geometry whose D is no multiple of 4: the scalar rows_expand1 / rows_collect1 kernels
ALL_GEOMS = GEOMS + [("odd", [5, 6, 7], [3, 3, 5], [6, 7])]
GEOM_IDS = [g[0] for g in ALL_GEOMS]
SPEC = GEOMS[1]


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------- kernels through the C ABI
SENTINEL = -7.5


def np_rank(n, share, seed):
    """live flags of n positions (share 0 / 1: none / all) -> (live, rank [n + 1])"""
    rs = np.random.RandomState(seed)
    live = np.zeros(n, bool) if share == 0 else (np.ones(n, bool) if share == 1 else rs.rand(n) < share)
    return live, np.concatenate([[0], np.cumsum(live)]).astype(np.int64)


def raw_rows(name, n, D, rank, src, offset_floats=0):
    """one of the two entry points through the raw C ABI into a destination full of SENTINEL; offset_floats: source and
    destination start that many floats behind a 16-byte boundary"""
    import tt_embeddings as E

    lib = E.lib()
    o = offset_floats
    s = torch.empty(n * D + o, dtype=torch.float32, device=DEV)
    s[o:].copy_(t(src).reshape(-1))
    d = torch.full((n * D + o,), SENTINEL, dtype=torch.float32, device=DEV)
    assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
    r = t(rank)
    rc = getattr(lib, name)(n, D, r.data_ptr(), s.data_ptr() + 4 * o, d.data_ptr() + 4 * o, stream())
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert (got[:o] == SENTINEL).all(), "wrote in front of the destination"
    return got[o:].reshape(n, D)


@pytest.mark.parametrize("n", [1, 63, 1025, 40000])
@pytest.mark.parametrize("D", [4, 45, 64, 260])
@pytest.mark.parametrize("share", [0, 0.5, 1])
def test_rows_kernels_vs_numpy(n, D, share):
    live, rank = np_rank(n, share, n + D)
    nl = int(rank[-1])
    rs = np.random.RandomState(D)
    rows = rs.standard_normal((n, D)).astype(np.float32)
    want = np.zeros((n, D), np.float32)
    want[live] = rows[:nl]
    runs = [raw_rows("ttx_rows_expand", n, D, rank, rows) for _ in range(2)]
    assert np.array_equal(runs[0], want), "expand: rows at their positions, exact zeros at the padding, every element written"
    assert np.array_equal(runs[0], runs[1])
    d_out = rs.standard_normal((n, D)).astype(np.float32)
    want = np.full((n, D), SENTINEL, np.float32)
    want[:nl] = d_out[live]
    runs = [raw_rows("ttx_rows_collect", n, D, rank, d_out) for _ in range(2)]
    assert np.array_equal(runs[0], want), "collect: the live gradient rows in order, rows >= rank[n] untouched"
    assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("name", ["ttx_rows_expand", "ttx_rows_collect"])
def test_rows_kernels_with_a_float_pointer_offset_by_4_bytes(name):
    """D % 4 == 0 but the float pointers 4 bytes behind a 16-byte boundary: the scalar kernels"""
    n, D = 1025, 64
    live, rank = np_rank(n, 0.5, 3)
    nl = int(rank[-1])
    src = np.random.RandomState(4).standard_normal((n, D)).astype(np.float32)
    got = raw_rows(name, n, D, rank, src, offset_floats=1)
    if name == "ttx_rows_expand":
        want = np.zeros((n, D), np.float32)
        want[live] = src[:nl]
    else:
        want = np.full((n, D), SENTINEL, np.float32)
        want[:nl] = src[live]
    assert np.array_equal(got, want)
    assert np.array_equal(got, raw_rows(name, n, D, rank, src, offset_floats=1))


def test_rows_shim_round_trip():
    import tt_embeddings as E

    n, D = 300, 12
    live, rank = np_rank(n, 0.5, 8)
    nl = int(rank[-1])
    rows = np.random.RandomState(9).standard_normal((n, D)).astype(np.float32)
    out = E.rows_expand(t(rank), t(rows))
    assert out.shape == (n, D) and np.array_equal(out.cpu().numpy()[live], rows[:nl]) and not out.cpu().numpy()[~live].any()
    into = torch.full((n, D), SENTINEL, device=DEV)
    assert E.rows_expand(t(rank), t(rows), out=into) is into and torch.equal(into, out)
    back = E.rows_collect(t(rank), out)
    assert np.array_equal(back.cpu().numpy()[:nl], rows[:nl])
    # the rank of the compaction itself
    idx = np.where(live, 9, PAD).astype(np.int64)
    comp, off, n_live = E.bags_compact(t(idx), None, 1, PAD)
    assert np.array_equal(off.cpu().numpy(), rank) and int(n_live.item()) == nl


# ------------------------------------------------------------------------------------------------------------------ module
def padded_indices(seed, shape, E_, pad=PAD, share=0.3):
    """int64 [rows, cols]: about `share` padding, row 0 all padding, row 1 without any"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, E_, size=shape).astype(np.int64)
    idx[idx == pad] = pad + 1
    idx[rs.rand(*shape) < share] = pad
    idx[0] = pad
    idx[1] = np.where(idx[1] == pad, pad + 1, idx[1])
    return idx


def embedding(geom, cores, **kw):
    import tt_embeddings_ops as ops

    _, p, q, r = geom
    m = ops.TTEmbedding(int(np.prod(p)), int(np.prod(q)), r, p, q, weight_dist="uniform", device=DEV, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(t(src))
    return m


_REF = {}


def case(geom):
    """the shared case of a geometry, computed once and left unchanged: indices (3, 50), gradient, float64 reference and the fp32 oracle (for its
    own distance from float64) on the live positions"""
    name, p, q, r = geom
    if name not in _REF:
        E_, D = int(np.prod(p)), int(np.prod(q))
        cores = G.make_cores(11, 1, p, q, r, "signed")
        idx = padded_indices(12, (3, 50), E_)
        d_out = (np.random.RandomState(13).rand(3, 50, D) * 0.1).astype(np.float32)
        keep = idx.reshape(-1) != PAD
        live, n = idx.reshape(-1)[keep], int(keep.sum())
        ar, tb = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
        d_live = d_out.reshape(-1, D)[keep]
        ref = R64.forward_backward(1, p, q, r, n, live, ar, tb, cores, d_out=d_live[None])
        g = O.make_geom(1, p, q, r)
        o_out = O.tt_forward(g, n, D, live, ar, tb, cores)[0]
        o_g = O.tt_backward(g, O.OPTIM_DENSE, n, D, 0, 0, live, ar, tb, d_live[None], [np.array(c, copy=True) for c in cores])
        _REF[name] = dict(cores=cores, idx=idx, d_out=d_out, keep=keep, ref=ref, o_out=o_out, o_g=o_g)
    return _REF[name]


def close64(got, want, oracle, what):
    f, u = R64.widen_factor(oracle, want)
    print(f"[unpooled] {what}: {R64.default_units(got, want):.3f} default bounds from float64 (the fp32 oracle: {u:.3f}, bound x{f:.2f})")
    assert_close(got, want, what, rtol=RTOL * f, atol_scale=ATOL_SCALE * f)
    return f


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=GEOM_IDS)
def test_forward_and_dense_gradients_vs_float64(geom):
    c = case(geom)
    m = embedding(geom, c["cores"], sparse=False, padding_idx=PAD)
    out = m(t(c["idx"]))
    D = c["d_out"].shape[-1]
    assert out.shape == (3, 50, D)
    got = out.detach().cpu().numpy().reshape(-1, D)
    assert not got[~c["keep"]].any(), "padding positions are exact zeros"
    close64(got[c["keep"]], c["ref"]["out"][0], c["o_out"], f"{geom[0]} forward")
    out.backward(t(c["d_out"]))
    for k in range(len(geom[1])):
        close64(m.tt_cores[k].grad.cpu().numpy(), c["ref"]["grads"][k], c["o_g"][k], f"{geom[0]} grad{k}")


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=GEOM_IDS)
def test_fused_sgd_step_vs_float64(geom):
    import tt_embeddings_ops as ops

    c = case(geom)
    m = embedding(geom, c["cores"], sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=PAD)
    m(t(c["idx"])).backward(t(c["d_out"]))
    want = R64.sgd_step(c["cores"], c["ref"]["grads"], LR)
    for k in range(len(geom[1])):
        o_w = c["cores"][k] - np.float32(LR) * c["o_g"][k]
        close64(m.tt_cores[k].detach().cpu().numpy(), want[k], o_w, f"{geom[0]} sgd core{k}")


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=GEOM_IDS)
def test_fused_adagrad_step_vs_float64(geom):
    import tt_embeddings_ops as ops

    c = case(geom)
    ref = c["ref"]
    m = embedding(geom, c["cores"], sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=LR, eps=EPS, padding_idx=PAD)
    state0 = [np.zeros_like(x) for x in c["cores"]]
    m(t(c["idx"])).backward(t(c["d_out"]))
    e_w, e_s = R64.adagrad_step(c["cores"], state0, ref["grads"], ref["touched"], LR, EPS)
    for k in range(len(geom[1])):
        f, _ = R64.widen_factor(c["o_g"][k], ref["grads"][k])
        R64.assert_state_close(m.optimizer_state[k].cpu().numpy(), e_s[k], ref["grads"][k], f"{geom[0]} adagrad state{k}", scale=f)
        assert_adagrad_close(m.tt_cores[k].detach().cpu().numpy(), e_w[k], ref["grads"][k], f"{geom[0]} adagrad core{k}", lr=LR,
                             eps=EPS, scale=f)


# ----------------------------------------------------------------------------------------------------------- bit identities
UNSPLIT = [g for g in ALL_GEOMS if g[0] != "q8"]  # (q0 = 8 takes the part lookups: held against the unsplit route in its own test)


@pytest.mark.parametrize("geom", UNSPLIT, ids=[g[0] for g in UNSPLIT])
def test_output_is_the_engines_rows_bit_for_bit(geom):
    """(a) without padding: tt_rows of the same indices; (b) with padding: (a)'s rows at the live positions, 0.0 elsewhere"""
    import tt_embeddings as E

    _, p, q, r = geom
    c = case(geom)
    D = c["d_out"].shape[-1]
    idx = t(c["idx"])
    rows = E.tt_rows(1, D, p, q, [1] + r + [1], idx.reshape(-1), None, [t(x) for x in c["cores"]])
    a = embedding(geom, c["cores"])(idx)
    assert torch.equal(a.detach().reshape(-1, D), rows)
    b = embedding(geom, c["cores"], padding_idx=PAD)(idx).detach().reshape(-1, D)
    keep = t(c["keep"])
    assert torch.equal(b[keep], rows[keep])
    assert (b[~keep] == 0.0).all() and not torch.signbit(b[~keep]).any()


@pytest.mark.parametrize("geom", ALL_GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_fused_step_equals_the_step_on_the_hand_compacted_batch(geom, optim):
    """(c) the same module fed indices[keep] with d_out[keep]: bit-identical cores (and state)"""
    import tt_embeddings_ops as ops

    c = case(geom)
    D = c["d_out"].shape[-1]
    kw = dict(sparse=True, learning_rate=LR, eps=EPS, optimizer=ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD)
    a, b = embedding(geom, c["cores"], padding_idx=PAD, **kw), embedding(geom, c["cores"], padding_idx=PAD, **kw)
    a(t(c["idx"])).backward(t(c["d_out"]))
    keep = c["keep"]
    b(t(c["idx"].reshape(-1)[keep])).backward(t(c["d_out"].reshape(-1, D)[keep]))
    for k in range(len(geom[1])):
        assert torch.equal(a.tt_cores[k], b.tt_cores[k]), f"core {k}"
        assert torch.equal(a.optimizer_state[k], b.optimizer_state[k]), f"state {k}"
    assert not torch.equal(a.tt_cores[0], t(c["cores"][0]))


@pytest.mark.parametrize("pad", [None, PAD], ids=["plain", "padded"])
def test_dedup_output_is_bit_identical_and_its_gradients_match_float64(pad):
    """(d) a batch with repeats: indices drawn from 20 distinct values"""
    _, p, q, r = SPEC
    E_, D = int(np.prod(p)), 64
    rs = np.random.RandomState(21)
    cores = G.make_cores(22, 1, p, q, r, "signed")
    values = rs.choice(np.arange(10, E_), size=20, replace=False)
    idx = values[rs.randint(0, 20, size=(3, 50))].astype(np.int64)
    if pad is not None:
        idx[rs.rand(3, 50) < 0.3] = pad
    d_out = (rs.rand(3, 50, D) * 0.1).astype(np.float32)
    plain = embedding(SPEC, cores, sparse=False, padding_idx=pad)
    dd = embedding(SPEC, cores, sparse=False, padding_idx=pad, dedup=True)
    oa, ob = plain(t(idx)), dd(t(idx))
    assert torch.equal(oa, ob), "dedup=True output differs from dedup=False"
    ob.backward(t(d_out))
    keep = idx.reshape(-1) != pad if pad is not None else np.ones(idx.size, bool)
    live, n = idx.reshape(-1)[keep], int(keep.sum())
    ar, tb = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
    d_live = d_out.reshape(-1, D)[keep]
    ref = R64.forward_backward(1, p, q, r, n, live, ar, tb, cores, d_out=d_live[None])
    o_g = O.tt_backward(O.make_geom(1, p, q, r), O.OPTIM_DENSE, n, D, 0, 0, live, ar, tb, d_live[None], [np.array(c, copy=True) for c in cores])
    for k in range(3):
        close64(dd.tt_cores[k].grad.cpu().numpy(), ref["grads"][k], o_g[k], f"dedup grad{k}")


def test_split_route_matches_the_unsplit_route(monkeypatch):
    """(e) q = [8, 4, 4]: the part lookups of the core-0 row split against the unsplit geometry on the generic kernels"""
    import tt_embeddings_ops as ops

    geom = GEOMS[4]
    assert geom[0] == "q8" and geom[2] == [8, 4, 4]
    c = case(geom)
    D = c["d_out"].shape[-1]
    res = {}
    for route in ("split", "unsplit"):
        if route == "unsplit":
            monkeypatch.setenv("TTX_NO_SPLIT0", "1")
        for pad in (None, PAD):
            m = embedding(geom, c["cores"], sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=pad)
            assert m._split0 == (2 if route == "split" else 0), "the split route was not taken"
            out = m(t(c["idx"]))
            out.backward(t(c["d_out"]))
            res[route, pad] = [out.detach().cpu().numpy()] + [x.detach().cpu().numpy() for x in m.tt_cores]
    keep = c["keep"]
    for pad in (None, PAD):
        for k, (a, b) in enumerate(zip(res["split", pad], res["unsplit", pad])):
            assert_close(a, b, f"split vs unsplit, padding_idx={pad}, {'output' if k == 0 else f'core{k - 1}'}")
    got = res["split", PAD][0].reshape(-1, D)
    assert not got[~keep].any()
    close64(got[keep], c["ref"]["out"][0], c["o_out"], "q8 split forward")


# ------------------------------------------------------------------------------------------------- sizes that switch routes
@pytest.mark.parametrize("N", [1, 40000])
def test_sizes_that_switch_routes(N):
    """N = 40,000 with padding: past the compaction's one-launch limit (32,768) and the duplicate map's 16,384; N = 1"""
    import tt_embeddings as E
    import tt_embeddings_ops as ops

    _, p, q, r = SPEC
    E_, D = int(np.prod(p)), 64
    cores = G.make_cores(31, 1, p, q, r, "signed")
    rs = np.random.RandomState(32)
    idx = rs.randint(10, E_, size=N).astype(np.int64)
    if N > 1:
        idx[rs.rand(N) < 0.3] = PAD
    keep = idx != PAD
    d_out = (rs.rand(N, D) * 0.1).astype(np.float32)
    rows = E.tt_rows(1, D, p, q, [1] + r + [1], t(idx), None, [t(x) for x in cores])
    kw = dict(sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=PAD)
    a, b, dd = embedding(SPEC, cores, **kw), embedding(SPEC, cores, **kw), embedding(SPEC, cores, dedup=True, **kw)
    oa = a(t(idx))
    assert torch.equal(oa.detach()[t(keep)], rows[t(keep)]) and not oa.detach()[t(~keep)].any()
    assert torch.equal(dd(t(idx)), oa)
    oa.backward(t(d_out))
    b(t(idx[keep])).backward(t(d_out[keep]))
    for k in range(3):
        assert torch.equal(a.tt_cores[k], b.tt_cores[k]), f"core {k} vs the hand-compacted batch"


@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_all_padding_batch_gives_zeros_and_changes_nothing(optim):
    import tt_embeddings_ops as ops

    cores = G.make_cores(41, 1, SPEC[1], SPEC[2], SPEC[3], "signed")
    m = embedding(SPEC, cores, sparse=True, learning_rate=LR, eps=EPS, padding_idx=PAD,
                  optimizer=ops.OptimType.SGD if optim == "sgd" else ops.OptimType.EXACT_ADAGRAD)
    if optim == "adagrad":
        with torch.no_grad():
            for s in m.optimizer_state:
                s.fill_(0.125)
    before = [x.detach().clone() for x in m.tt_cores] + [s.clone() for s in m.optimizer_state]
    out = m(torch.full((3, 50), PAD, dtype=torch.int64, device=DEV))
    assert out.shape == (3, 50, 64) and not out.any()
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    after = [x.detach() for x in m.tt_cores] + list(m.optimizer_state)
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_empty_input():
    cores = G.make_cores(42, 1, SPEC[1], SPEC[2], SPEC[3], "signed")
    for pad in (None, PAD):
        m = embedding(SPEC, cores, sparse=False, padding_idx=pad)
        out = m(torch.zeros((4, 0), dtype=torch.int64, device=DEV))
        assert out.shape == (4, 0, 64) and out.is_cuda
        out.backward(torch.zeros_like(out))
        assert all(x.grad is not None and not x.grad.any() for x in m.tt_cores)


# --------------------------------------------------------------------------------------------------- capture, determinism
def test_captured_padded_step_replays_bit_identically_to_eager_steps():
    """one capture over a static (8, 64) input; three batches with 10 %, 60 % and 0 % padding copied into it between replays:
    the live count is not baked into the graph"""
    import tt_embeddings_ops as ops
    import ttx_graph

    _, p, q, r = SPEC
    E_ = int(np.prod(p))
    cores = G.make_cores(51, 1, p, q, r, "signed")
    example = padded_indices(52, (8, 64), E_, share=0.3)
    batches = [padded_indices(53, (8, 64), E_, share=0.1), padded_indices(54, (8, 64), E_, share=0.6),
               np.where(padded_indices(55, (8, 64), E_, share=0.0) == PAD, PAD + 1, padded_indices(55, (8, 64), E_, share=0.0))]
    assert not (batches[2] == PAD).any() and len({int((b == PAD).sum()) for b in batches}) == 3
    g = t((np.random.RandomState(56).rand(8, 64, 64) * 0.1).astype(np.float32))
    outs = {False: [], True: []}

    def run(graphed):
        m = embedding(SPEC, cores, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=LR, padding_idx=PAD)
        seen = torch.zeros(8, 64, 64, device=DEV)

        def step(i, d):
            out = m(i)
            seen.copy_(out.detach())
            out.backward(d)

        if graphed:
            gs = ttx_graph.GraphedStep(step, (t(example), g), warmup=2)
        else:
            for _ in range(2):
                step(t(example), g)
        for bt in batches:
            if graphed:
                gs(t(bt), g)
            else:
                step(t(bt), g)
            torch.cuda.synchronize()
            outs[graphed].append(seen.clone())
        return [x.detach().clone() for x in m.tt_cores]

    eager, replayed = run(False), run(True)
    for k in range(3):
        assert torch.equal(eager[k], replayed[k]), f"core {k} differs between replay and eager"
    for a, b, bt in zip(outs[False], outs[True], batches):
        assert torch.equal(a, b), "output differs between replay and eager"
        assert not b[t(bt == PAD)].any() and b[t(bt != PAD)].abs().sum() > 0


def test_padded_adagrad_step_is_bit_deterministic():
    import tt_embeddings_ops as ops

    _, p, q, r = SPEC
    cores = G.make_cores(61, 1, p, q, r, "signed")
    idx = padded_indices(62, (16, 128), 3000)  # (a small key space: slices shared by many lookups)
    d = t((np.random.RandomState(63).rand(16, 128, 64) * 0.1).astype(np.float32))
    runs = []
    for _ in range(2):
        m = embedding(SPEC, cores, sparse=True, optimizer=ops.OptimType.EXACT_ADAGRAD, learning_rate=LR, eps=EPS, padding_idx=PAD)
        m(t(idx)).backward(d)
        torch.cuda.synchronize()
        runs.append([x.detach().clone() for x in m.tt_cores] + [s.clone() for s in m.optimizer_state])
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    assert runs[0][3].any()


# ------------------------------------------------------------------------------------------------------------- refusals
def test_dedup_with_padding_refuses_capture(monkeypatch):
    cores = G.make_cores(71, 1, SPEC[1], SPEC[2], SPEC[3], "signed")
    m = embedding(SPEC, cores, sparse=False, padding_idx=PAD, dedup=True)
    idx = t(padded_indices(72, (3, 50), 1000))
    with monkeypatch.context() as mp:  # (as if a capture were under way: nothing is captured, nothing left behind on the device)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="live count is read back"):
            m(idx)
    assert m(idx).shape == (3, 50, 64)  # (eagerly it is served)
