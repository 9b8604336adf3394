"""GPU tests of the unpooled lookup with a LIVE row cache, `TTEmbedding(use_cache=True)` after cache_populate(): the two byte
movers ttx_rows_place / ttx_rows_pick through the raw C ABI against numpy, and the module -- forward against the float64 rows,
one dense / fused SGD / fused Adagrad step with the cores against tt_ref64 driven by the MISS positions only and the cache rows
against a numpy restatement built from the module's own hash table, agreement with TTEmbeddingBag(use_cache=True) fed one bag
per position, warm-up counting, the edges, capture and determinism."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
import tt_ref64 as R64
from test_pooling_modes_gpu import GEOMS, t
from test_unpooled_gpu import ALL_GEOMS
from util import ATOL_SCALE, EPS, LR, RTOL, assert_adagrad_close, assert_close, rowwise_adagrad_segments_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 5
SENTINEL = -7.5
MODULE_GEOMS = [g for g in GEOMS if g[0] in ("spec", "q8")] + [g for g in ALL_GEOMS if g[0] == "odd"]
MODULE_IDS = [g[0] for g in MODULE_GEOMS]
assert MODULE_IDS == ["spec", "q8", "odd"]
# the row-wise Adagrad state and rows of the cache: the bound tests/test_cache_routes_gpu.py and tests/test_cache_gpu.py hold them to
# at every size (the state is a running fp32 sum in another association than the reference's, every step's size comes from it)
ADAGRAD_TOL = dict(rtol=2e-5, atol_scale=4e-6)


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------- kernels through the C ABI
CS = 37  # cache rows of the kernel cases


def np_batch(N, D, pad_share, hit_share, seed):
    """N positions, `pad_share` of them padding; the n live ones in a random partition order, `hit_share` of them hits"""
    rs = np.random.RandomState(seed)
    live = np.ones(N, bool) if pad_share == 0 else (np.zeros(N, bool) if pad_share == 1 else rs.rand(N) >= pad_share)
    rank = np.concatenate([[0], np.cumsum(live)]).astype(np.int64)
    pos = rs.permutation(np.nonzero(live)[0]).astype(np.int64)
    n = pos.size
    n_tt = n if hit_share == 0 else (0 if hit_share == 1 else n - n // 2)
    loc = np.full(n, -1, np.int32)
    loc[n_tt:] = rs.randint(0, CS, size=n - n_tt)
    rows_tt = rs.standard_normal((max(n, 1), D)).astype(np.float32)
    cache = rs.standard_normal((CS, D)).astype(np.float32)
    d_out = rs.standard_normal((N, D)).astype(np.float32)
    return dict(N=N, D=D, n=n, n_tt=n_tt, live=live, rank=rank, pos=pos, loc=loc, rows_tt=rows_tt, cache=cache, d_out=d_out)


def dev_floats(a, o):
    """`a` on the device, starting o floats behind a 16-byte boundary -> (tensor that owns the memory, address of the data)"""
    buf = torch.empty(a.size + o, dtype=torch.float32, device=DEV)
    buf[o:].copy_(t(a).reshape(-1))
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 4 * o


def raw_place(c, on_device, with_rank, o=0):
    import tt_embeddings as E

    lib = E.lib()
    N, D, n = c["N"], c["D"], c["n"]
    pos, loc = t(c["pos"]), t(c["loc"])
    rank = t(c["rank"]) if with_rank else None
    rows, rows_p = dev_floats(c["rows_tt"], o)
    cache, cache_p = dev_floats(c["cache"], o)
    out = torch.full((N * D + o,), SENTINEL, dtype=torch.float32, device=DEV)
    split = torch.tensor([c["n_tt"]], dtype=torch.int32, device=DEV) if on_device else None
    rc = lib.ttx_rows_place(N, n, n if on_device else c["n_tt"], None if split is None else split.data_ptr(), D,
                            pos.data_ptr() if n else None, loc.data_ptr() if n else None, rows_p, cache_p, CS,
                            None if rank is None else rank.data_ptr(), out.data_ptr() + 4 * o, stream())
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[:o] == SENTINEL).all(), "wrote in front of the destination"
    return got[o:].reshape(N, D)


def raw_pick(c, on_device, o=0):
    import tt_embeddings as E

    lib = E.lib()
    N, D, n = c["N"], c["D"], c["n"]
    pos = t(c["pos"])
    d_out, d_out_p = dev_floats(c["d_out"], o)
    d_rows = torch.full((N * D + o,), SENTINEL, dtype=torch.float32, device=DEV)
    split = torch.tensor([c["n_tt"]], dtype=torch.int32, device=DEV) if on_device else None
    rc = lib.ttx_rows_pick(N, n, n if on_device else c["n_tt"], None if split is None else split.data_ptr(), D,
                           pos.data_ptr() if n else None, d_out_p, d_rows.data_ptr() + 4 * o, stream())
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    got = d_rows.cpu().numpy()
    assert (got[:o] == SENTINEL).all(), "wrote in front of the destination"
    return got[o:].reshape(N, D)


def check_kernels(c, o=0):
    N, D, n, n_tt = c["N"], c["D"], c["n"], c["n_tt"]
    want = np.full((N, D), SENTINEL, np.float32)
    want[~c["live"]] = 0.0
    want[c["pos"][:n_tt]] = c["rows_tt"][:n_tt]
    want[c["pos"][n_tt:]] = c["cache"][c["loc"][n_tt:]]
    assert not (want == SENTINEL).any()
    want_pick = np.full((N, D), SENTINEL, np.float32)
    want_pick[:n_tt] = c["d_out"][c["pos"][:n_tt]]
    for on_device in (True, False):
        ranks = (True, False) if n == N else (True,)  # (no padding: with the rank of an unpadded batch and with rank == NULL)
        for with_rank in ranks:
            runs = [raw_place(c, on_device, with_rank, o) for _ in range(2)]
            assert np.array_equal(runs[0], want), "place: rows at their positions, exact zeros at the padding, every element written"
            assert np.array_equal(runs[0], runs[1])
        runs = [raw_pick(c, on_device, o) for _ in range(2)]
        assert np.array_equal(runs[0], want_pick), "pick: the misses' gradient rows in partition order, rows >= n_tt untouched"
        assert np.array_equal(runs[0], runs[1])


@pytest.mark.parametrize("N", [1, 63, 1025, 40000])
@pytest.mark.parametrize("D", [4, 45, 64, 260])
@pytest.mark.parametrize("pad_share", [0, 0.5, 1])
def test_place_and_pick_vs_numpy(N, D, pad_share):
    for hit_share in (0, 0.5, 1):
        check_kernels(np_batch(N, D, pad_share, hit_share, N + D + int(10 * hit_share)))


def test_place_and_pick_with_the_float_pointers_offset_by_4_bytes():
    """D % 4 == 0 but the float pointers 4 bytes behind a 16-byte boundary: the scalar kernels"""
    check_kernels(np_batch(1025, 64, 0.5, 0.5, 3), o=1)


def test_shim_round_trip():
    import tt_embeddings as E

    c = np_batch(300, 12, 0.5, 0.5, 8)
    split = torch.tensor([c["n_tt"]], dtype=torch.int32, device=DEV)
    for n_tt in (split, c["n_tt"]):
        out = E.rows_place(300, n_tt, t(c["pos"]), t(c["loc"]), t(c["rows_tt"]), t(c["cache"]), t(c["rank"]))
        got = out.cpu().numpy()
        assert not got[~c["live"]].any() and np.array_equal(got[c["pos"][:c["n_tt"]]], c["rows_tt"][:c["n_tt"]])
        assert np.array_equal(got[c["pos"][c["n_tt"]:]], c["cache"][c["loc"][c["n_tt"]:]])
        back = E.rows_pick(n_tt, t(c["pos"]), out)
        assert np.array_equal(back.cpu().numpy()[:c["n_tt"]], c["rows_tt"][:c["n_tt"]])


# ------------------------------------------------------------------------------------------------------------------ module
WARM = np.arange(10, 110, dtype=np.int64)  # the keys the cache warms up on (PAD is not among them); 120 .. E - 1 are never counted


def make(geom, cores, cls="emb", **kw):
    import tt_embeddings_ops as ops

    _, p, q, r = geom
    kw = dict(dict(use_cache=True, cache_size=128, hashtbl_size=1024, weight_dist="uniform", device=DEV), **kw)
    ctor = ops.TTEmbedding if cls == "emb" else ops.TTEmbeddingBag
    m = ctor(int(np.prod(p)), int(np.prod(q)), r, p, q, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(t(src))
    return m


def call(m, idx):
    """the module on a batch of positions: TTEmbedding as it is, the bag module with one bag per position"""
    import tt_embeddings_ops as ops

    if isinstance(m, ops.TTEmbedding):
        return m(idx)
    flat = idx.reshape(-1)
    return m(flat, torch.arange(flat.numel() + 1, device=DEV)).view(tuple(idx.shape) + (-1,))


def go_live(m):
    """about 100 warm-up keys into 128 cache rows of a 1024-slot table: populate evicts nothing, so the hash table's layout
    (which concurrent inserts leave to arrival order) cannot move a cached key"""
    with torch.no_grad():
        call(m, t(WARM))
    m.cache_populate()
    assert not m.warmup
    return m


def cached_rows(m):
    """{key: cache row} from the module's own hash table"""
    ht, cs = m.hashtbl.cpu().numpy(), m.cache_state.cpu().numpy()
    return {int(ht[s]): int(cs[s]) for s in range(ht.size) if ht[s] >= 0 and cs[s] >= 0}


def step_batch(geom, seed, shape=(6, 40), padded=False, hit_share=0.5):
    """warm-up keys (hits) mixed with keys never counted (misses); padded: about 30 % PAD and row 0 all padding"""
    E_ = int(np.prod(geom[1]))
    rs = np.random.RandomState(seed)
    idx = np.where(rs.rand(*shape) < hit_share, WARM[rs.randint(0, WARM.size, size=shape)],
                   rs.randint(120, E_, size=shape)).astype(np.int64)
    if padded:
        idx[rs.rand(*shape) < 0.3] = PAD
        idx[0] = PAD
    return idx


_CASES = {}


def case(geom, padded):
    """the shared case of (geometry, padded), computed once and left unchanged: cores, the step's batch (6, 40), its gradient and --
    given the keys that are cached -- the float64 reference of the miss positions and the fp32 oracle's own distance from it"""
    key = (geom[0], padded)
    if key not in _CASES:
        _, p, q, r = geom
        D = int(np.prod(q))
        cores = G.make_cores(21, 1, p, q, r, "signed")
        idx = step_batch(geom, 22 + padded, padded=padded)
        d_out = (np.random.RandomState(23).rand(*idx.shape, D) * 0.1).astype(np.float32)
        _CASES[key] = dict(cores=cores, idx=idx, d_out=d_out, refs={})
    return _CASES[key]


def reference(geom, c, loc_of):
    """float64 forward of every live position and forward + backward of the MISS positions only (one bag each), the fp32 oracle
    on the same misses; shared by the cases whose modules cache the same keys"""
    _, p, q, r = geom
    D = int(np.prod(q))
    flat = c["idx"].reshape(-1)
    live = flat != PAD if (flat == PAD).any() else np.ones(flat.size, bool)
    hit = np.array([int(v) in loc_of for v in flat]) & live
    miss = live & ~hit
    key = (hit.tobytes(), tuple(sorted(loc_of.items())))
    if key not in c["refs"]:
        cores = c["cores"]
        d = c["d_out"].reshape(-1, D)

        def run(mask, with_grad):
            n = int(mask.sum())
            ar, tb = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
            ref = R64.forward_backward(1, p, q, r, n, flat[mask], ar, tb, cores, d_out=d[mask][None] if with_grad else None)
            if not with_grad:
                return ref, None
            g = O.make_geom(1, p, q, r)
            o_g = O.tt_backward(g, O.OPTIM_DENSE, n, D, 0, 0, flat[mask], ar, tb, d[mask][None], [np.array(x, copy=True) for x in cores])
            return ref, o_g

        fwd, _ = run(live, False)
        ref, o_g = run(miss, True)
        c["refs"][key] = dict(live=live, hit=hit, miss=miss, out=fwd["out"][0], ref=ref, o_g=o_g,
                              loc=np.array([loc_of.get(int(v), -1) for v in flat]))
    return c["refs"][key]


_LIVE = {}


def live_module(geom, padded, optim, det=None, cls="emb"):
    """a module of class `cls` whose cache is live.  The state is built once per (geometry, optimizer) -- a TTEmbedding warmed up
    and populated -- and every case gets a copy of it (state_dict() is the bag module's, so it loads into either class): which of
    two colliding keys takes which slot of the hash table is left to arrival order, and modules warmed up one by one could
    disagree about it, which bit comparisons between two modules must not depend on."""
    import tt_embeddings_ops as ops

    c = case(geom, padded)
    optimizer = {"dense": None, "sgd": ops.OptimType.SGD, "adagrad": ops.OptimType.EXACT_ADAGRAD}[optim]
    kw = dict(sparse=optimizer is not None, optimizer=optimizer or ops.OptimType.SGD, learning_rate=LR, eps=EPS)
    key = (geom[0], optim)
    if key not in _LIVE:
        m = go_live(make(geom, c["cores"], "emb", **kw))
        if m.cache_optimizer_state is not None:  # a state that is not all zero: the step sizes depend on it
            m.cache_optimizer_state.view(-1)[:128] = t((np.random.RandomState(3).rand(128) * 0.01).astype(np.float32))
        _LIVE[key] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = make(geom, c["cores"], cls, padding_idx=PAD if padded else None, deterministic_cache_update=det, **kw)
    m.load_state_dict(_LIVE[key])
    m.warmup = False
    return m, c


def assert_mixed(rf, padded, idx):
    n_hit, n_live = int(rf["hit"].sum()), int(rf["live"].sum())
    assert 0 < n_hit < n_live, f"the batch must mix hits and misses ({n_hit} hits of {n_live} live positions)"
    if padded:
        assert (idx == PAD).any() and (idx == PAD).all(axis=1).any(), "padding, one all-padding row included"


def close64(got, want, oracle, what):
    f, u = R64.widen_factor(oracle, want)
    print(f"[unpooled cache] {what}: {R64.default_units(got, want):.3f} default bounds from float64 (the fp32 oracle: {u:.3f}, bound x{f:.2f})")
    assert_close(got, want, what, rtol=RTOL * f, atol_scale=ATOL_SCALE * f)


@pytest.mark.parametrize("geom", MODULE_GEOMS, ids=MODULE_IDS)
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
@pytest.mark.parametrize("optim", ["dense", "sgd", "adagrad"])
def test_cache_live_step_vs_float64(geom, padded, optim):
    # (Adagrad: the sorted update, whose order within a cache row is defined -- the atomic one's is arrival order, as in the reference)
    m, c = live_module(geom, padded, optim, det=True if optim == "adagrad" else None)
    tag = f"{geom[0]} {'padded' if padded else 'plain'} {optim}: "
    D = c["d_out"].shape[-1]
    loc_of = cached_rows(m)
    rf = reference(geom, c, loc_of)
    assert_mixed(rf, padded, c["idx"])
    cw0 = m.cache_weight.detach().clone()
    cst0 = None if m.cache_optimizer_state is None else m.cache_optimizer_state.detach().clone()
    out = m(t(c["idx"]))
    assert out.shape == c["idx"].shape + (D,)
    got = out.detach().cpu().numpy().reshape(-1, D)
    # ---- forward: F.embedding(idx, W0) on the float64 table; the hits are their cache rows to the bit, the padding exact zeros
    assert_close(got[rf["live"]], rf["out"], tag + "forward")
    assert np.array_equal(got[rf["hit"]], cw0.cpu().numpy()[rf["loc"][rf["hit"]]]), "a hit is its cache row"
    assert not got[~rf["live"]].any(), "padding positions are exact zeros"
    out.backward(t(c["d_out"]))
    torch.cuda.synchronize()
    # ---- the cores: tt_ref64 driven with the miss positions only
    ref, o_g, cores = rf["ref"], rf["o_g"], c["cores"]
    T = len(geom[1])
    if optim == "dense":
        for k in range(T):
            close64(m.tt_cores[k].grad.cpu().numpy(), ref["grads"][k], o_g[k], tag + f"grad{k}")
    elif optim == "sgd":
        want = R64.sgd_step(cores, ref["grads"], LR)
        for k in range(T):
            close64(m.tt_cores[k].detach().cpu().numpy(), want[k], cores[k] - np.float32(LR) * o_g[k], tag + f"sgd core{k}")
    else:
        e_w, e_s = R64.adagrad_step(cores, [np.zeros_like(x) for x in cores], ref["grads"], ref["touched"], LR, EPS)
        for k in range(T):
            f, _ = R64.widen_factor(o_g[k], ref["grads"][k])
            R64.assert_state_close(m.optimizer_state[k].cpu().numpy(), e_s[k], ref["grads"][k], tag + f"adagrad state{k}", scale=f)
            assert_adagrad_close(m.tt_cores[k].detach().cpu().numpy(), e_w[k], ref["grads"][k], tag + f"adagrad core{k}", lr=LR,
                                 eps=EPS, scale=f)
    # ---- the cache rows: a numpy restatement from hashtbl / cache_state
    d = c["d_out"].reshape(-1, D).astype(np.float64)
    hits = np.nonzero(rf["hit"])[0][::-1]  # (the order the partition leaves the hits in: behind the misses, reversed)
    touched = np.zeros(128, bool)
    touched[rf["loc"][hits]] = True
    untouched = t(~touched)
    if optim == "dense":
        want = np.zeros((128, D))
        np.add.at(want, rf["loc"][hits], d[hits])
        g = m.cache_weight.grad
        assert_close(g.cpu().numpy(), want, tag + "cache row gradient")
        assert not bool(g[untouched].any()), "the gradient of rows nobody hit must be exactly zero"
        assert torch.equal(m.cache_weight.detach(), cw0)
        return
    cw = m.cache_weight.detach()
    assert torch.equal(cw[untouched], cw0[untouched]), "rows nobody hit must not change by a bit"
    if optim == "sgd":
        want = cw0.double().cpu().numpy()
        np.subtract.at(want, rf["loc"][hits], LR * d[hits])
        assert_close(cw.cpu().numpy(), want, tag + "cache rows after SGD")
        return
    st_got, st0 = m.cache_optimizer_state.detach().reshape(-1), cst0.reshape(-1)
    assert torch.equal(st_got[128:], st0[128:]), "the buffer behind the row-wise state must not be written"
    assert torch.equal(st_got[:128][untouched], st0[:128][untouched]), "the state of rows nobody hit must not change by a bit"
    st64, w64 = rowwise_adagrad_segments_f64(d[hits], rf["loc"][hits], np.arange(hits.size), LR, EPS, st0[:128].cpu().numpy(),
                                             cw0.cpu().numpy())
    assert_close(st_got[:128].cpu().numpy(), st64, tag + "cache optimizer state", **ADAGRAD_TOL)
    assert_close(cw.cpu().numpy(), w64, tag + "cache rows after row-wise Adagrad", **ADAGRAD_TOL)


@pytest.mark.parametrize("geom", MODULE_GEOMS, ids=MODULE_IDS)
@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_agrees_with_the_bag_module_fed_one_bag_per_position(geom, padded):
    res = {}
    for cls in ("emb", "bag"):
        m, c = live_module(geom, padded, "sgd", det=True, cls=cls)
        out = call(m, t(c["idx"]))
        out.backward(t(c["d_out"]))
        torch.cuda.synchronize()
        res[cls] = [out.detach().cpu().numpy(), m.cache_weight.detach().cpu().numpy()] + [x.detach().cpu().numpy() for x in m.tt_cores]
    for what, a, b in zip(["output", "cache rows", "core0", "core1", "core2"], res["emb"], res["bag"]):
        assert_close(a, b, f"{geom[0]} {what}: TTEmbedding vs TTEmbeddingBag")


@pytest.mark.parametrize("padded", [False, True], ids=["plain", "padded"])
def test_warm_up_counts_what_the_bag_module_counts(padded):
    """(a hash table of 2^16 slots for the batch's 200 keys: no key runs out of probes, which of two such keys is dropped being
    left to arrival order -- asserted: every live position is counted)"""
    geom = MODULE_GEOMS[0]
    c = case(geom, padded)
    live = int((c["idx"] != PAD).sum()) if padded else c["idx"].size
    pairs = {}
    for cls in ("emb", "bag"):
        m = make(geom, c["cores"], cls, padding_idx=PAD if padded else None, hashtbl_size=1 << 16)
        with torch.no_grad():
            call(m, t(c["idx"]))
        assert m.warmup
        ht, fr = m.hashtbl.cpu().numpy(), m.cache_freq.cpu().numpy()
        pairs[cls] = sorted(zip(ht[ht >= 0].tolist(), fr[ht >= 0].tolist()))
        assert sum(v for _, v in pairs[cls]) == live, "every live position is counted once"
    assert pairs["emb"] == pairs["bag"] and len(pairs["emb"]) > 50
    if padded:
        assert (c["idx"] == PAD).any() and PAD not in [k for k, _ in pairs["emb"]], "padding must not be counted"


# ------------------------------------------------------------------------------------------------------------------- edges
def snapshot(m, freq=True):
    """cores (0..2), their optimizer state (3..5), cache rows (6), [cache_freq,] [the cache rows' optimizer state]"""
    st = [] if m.cache_optimizer_state is None else [m.cache_optimizer_state]
    return [x.detach().clone() for x in list(m.tt_cores) + list(m.optimizer_state) + [m.cache_weight] + ([m.cache_freq] if freq else []) + st]


@pytest.mark.parametrize("edge", ["all-hit", "all-miss"])
def test_all_hit_and_all_miss_batches(edge):
    geom = MODULE_GEOMS[0]
    _, p, q, r = geom
    m, c = live_module(geom, False, "sgd", det=True)
    loc_of = cached_rows(m)
    idx = step_batch(geom, 31, hit_share=1.0 if edge == "all-hit" else 0.0)
    idx = np.where(np.isin(idx, list(loc_of)) | (edge == "all-miss"), idx, WARM[0] if WARM[0] in loc_of else next(iter(loc_of)))
    n_hit = int(np.isin(idx, list(loc_of)).sum())
    assert n_hit == (idx.size if edge == "all-hit" else 0)
    d_out = t((np.random.RandomState(32).rand(*idx.shape, 64) * 0.1).astype(np.float32))
    before = snapshot(m)
    out = m(t(idx))
    got = out.detach().cpu().numpy().reshape(-1, 64)
    n = idx.size
    ref = R64.forward_backward(1, p, q, r, n, idx.reshape(-1), np.arange(n), np.zeros(n, np.int64), c["cores"])
    assert_close(got, ref["out"][0], edge + " forward")
    out.backward(d_out)
    torch.cuda.synchronize()
    after = snapshot(m)
    if edge == "all-hit":  # the cores do not move by a bit, the cache rows do
        assert all(torch.equal(a, b) for a, b in zip(before[:3], after[:3]))
        want = before[6].double().cpu().numpy()
        np.subtract.at(want, [loc_of[int(v)] for v in idx.reshape(-1)], LR * d_out.double().cpu().numpy().reshape(-1, 64))
        assert_close(after[6].cpu().numpy(), want, "all-hit cache rows after SGD")
    else:  # the cache rows do not move by a bit, the cores do
        assert torch.equal(before[6], after[6])
        assert not all(torch.equal(a, b) for a, b in zip(before[:3], after[:3]))


@pytest.mark.parametrize("optim", ["sgd", "adagrad"])
def test_all_padding_batch_changes_nothing(optim):
    m, _ = live_module(MODULE_GEOMS[0], True, optim)
    before = snapshot(m)
    out = m(torch.full((3, 7), PAD, dtype=torch.int64, device=DEV))
    assert out.shape == (3, 7, 64) and not bool(out.any())
    out.backward(torch.ones_like(out))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(m))), "cores, Adagrad state, cache rows and cache_freq stay"


def test_empty_input_and_one_position():
    m, c = live_module(MODULE_GEOMS[0], False, "sgd")
    before = snapshot(m)
    out = m(torch.zeros((4, 0), dtype=torch.int64, device=DEV))
    assert out.shape == (4, 0, 64) and out.is_cuda
    out.backward(torch.zeros_like(out))
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(m)))
    loc_of = cached_rows(m)
    key = next(iter(loc_of))
    for idx, is_hit in ((torch.tensor(key, device=DEV), True), (torch.tensor([4321], device=DEV), False)):
        cw0 = m.cache_weight.detach().clone()
        out = m(idx)
        assert out.shape == tuple(idx.shape) + (64,)
        if is_hit:
            assert torch.equal(out.detach().reshape(-1), cw0[loc_of[key]])
        out.backward(torch.ones_like(out))
        torch.cuda.synchronize()
        moved = (m.cache_weight.detach() != cw0).any(dim=1)
        assert int(moved.sum()) == (1 if is_hit else 0) and (not is_hit or bool(moved[loc_of[key]]))


def test_forty_thousand_positions_deterministic():
    """N = 40000 on D = 45 (the scalar movers, the sort chain of the cache rows' update): forward to the bit -- a hit is its cache
    row, a miss the engine's own row --, the cache rows against the float64 restatement, the cores against tt_ref64 on the misses"""
    import tt_embeddings as E

    geom = MODULE_GEOMS[2]
    _, p, q, r = geom
    D = int(np.prod(q))
    m, c = live_module(geom, False, "sgd", det=True)
    loc_of = cached_rows(m)
    idx = step_batch(geom, 41, shape=(40000,))
    hit = np.isin(idx, list(loc_of))
    assert 0 < int(hit.sum()) < idx.size
    d_out = (np.random.RandomState(42).rand(idx.size, D) * 0.01).astype(np.float32)
    cw0 = m.cache_weight.detach().clone()
    rows = E.tt_rows(1, D, p, q, [1] + r + [1], t(idx), None, [x.detach() for x in m.tt_cores]).cpu().numpy()
    out = m(t(idx))
    got = out.detach().cpu().numpy()
    loc = np.array([loc_of.get(int(v), 0) for v in idx])
    assert np.array_equal(got[hit], cw0.cpu().numpy()[loc[hit]]) and np.array_equal(got[~hit], rows[~hit])
    out.backward(t(d_out))
    torch.cuda.synchronize()
    want = cw0.double().cpu().numpy()
    np.subtract.at(want, loc[hit], LR * d_out[hit].astype(np.float64))
    assert_close(m.cache_weight.detach().cpu().numpy(), want, "cache rows after SGD, 40000 positions")
    n = int((~hit).sum())
    ar, tb = np.arange(n, dtype=np.int64), np.zeros(n, np.int64)
    ref = R64.forward_backward(1, p, q, r, n, idx[~hit], ar, tb, c["cores"], d_out=d_out[~hit][None])
    o_g = O.tt_backward(O.make_geom(1, p, q, r), O.OPTIM_DENSE, n, D, 0, 0, idx[~hit], ar, tb, d_out[~hit][None],
                        [np.array(x, copy=True) for x in c["cores"]])
    want = R64.sgd_step(c["cores"], ref["grads"], LR)
    for k in range(3):
        close64(m.tt_cores[k].detach().cpu().numpy(), want[k], c["cores"][k] - np.float32(LR) * o_g[k], f"40000 positions sgd core{k}")


# --------------------------------------------------------------------------------------------------- capture, determinism
def test_captured_step_replays_bit_identically_to_eager_steps():
    """one capture of a fused-SGD cache-live step over a static (6, 40) input; three batches with about 10 %, 60 % and 0 % hits
    copied into it between replays: the hit / miss split is not baked into the graph"""
    import ttx_graph

    geom = MODULE_GEOMS[0]
    example = step_batch(geom, 51)
    batches = [step_batch(geom, 52, hit_share=0.1), step_batch(geom, 53, hit_share=0.6), step_batch(geom, 54, hit_share=0.0)]
    g = t((np.random.RandomState(56).rand(6, 40, 64) * 0.1).astype(np.float32))
    outs, shares = {False: [], True: []}, []

    def run(graphed):
        m, _ = live_module(geom, False, "sgd", det=True)
        if not graphed:
            keys = list(cached_rows(m))
            shares.extend(float(np.isin(b, keys).mean()) for b in batches)
        seen = torch.zeros(6, 40, 64, device=DEV)

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
        return [x.detach().clone() for x in list(m.tt_cores) + [m.cache_weight]]

    eager, replayed = run(False), run(True)
    assert 0.02 < shares[0] < 0.25 and 0.4 < shares[1] < 0.8 and shares[2] == 0.0, shares
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), f"{'cache_weight' if k == 3 else f'core {k}'} differs between replay and eager"
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b), "output differs between replay and eager"


def test_padded_cache_live_route_refuses_capture(monkeypatch):
    m, c = live_module(MODULE_GEOMS[0], True, "sgd")
    warm = make(MODULE_GEOMS[0], c["cores"], padding_idx=PAD)  # (still warming up: the live indices are counted after a read-back)
    idx = t(c["idx"])
    with monkeypatch.context() as mp:  # (as if a capture were under way: nothing is captured, nothing left behind on the device)
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="live count is read back.*not capturable"):
            m(idx)
        with pytest.raises(RuntimeError, match="live count is read back.*not capturable"):
            warm(idx)
    assert m(idx).shape == (6, 40, 64)  # (eagerly it is served)


def test_adagrad_step_is_bit_deterministic():
    runs = []
    for _ in range(2):
        m, c = live_module(MODULE_GEOMS[0], False, "adagrad", det=True)
        idx = step_batch(MODULE_GEOMS[0], 61, shape=(16, 128))  # (100 hot keys: cache rows shared by many lookups)
        d = t((np.random.RandomState(63).rand(16, 128, 64) * 0.1).astype(np.float32))
        m(t(idx)).backward(d)
        torch.cuda.synchronize()
        runs.append(snapshot(m, freq=False))  # (cores, state, cache rows, their state; the slot a NEW key is counted in is arrival order)
    names = ["core0", "core1", "core2", "state0", "state1", "state2", "cache_weight", "cache_optimizer_state"]
    differ = [nm for nm, a, b in zip(names, *runs) if not torch.equal(a, b)]
    assert not differ, f"two identical steps from identical state must leave identical bits: {differ} differ"
