"""The cache-live backward THROUGH THE MODULE at the batch sizes, row widths and settings that switch its route.

With a live row cache the backward updates the cache rows on one of three routes:

  float-atomic scatter kernels            default below the auto threshold, `deterministic_cache_update=False` always
  cache_update_owner_kernel, one launch   sorted, nnz <= 32,768, D % 4 == 0, D <= 256
  sort chain (cs_keys .. cs_apply)        sorted, anything else

"sorted" = `deterministic_cache_update=True`, or the default (None) from 65,536 lookups per batch (row-wise Adagrad) /
262,144 (SGD, dense) on.  tests/test_cache_gpu.py holds the three routes through the C ABI; here they are reached the way a
training step reaches them: TTEmbeddingBag -> autograd node (the C++ one and the reference-shaped Python one) -> partitioned
batch with the split point on the device -> (weighted: scaled gradient rows, iota) -> route.

Reference of every case: float64.  The cores are expanded to the full table in float64, the cached rows are laid over it,
torch's embedding_bag and autograd run on that.  Row-wise Adagrad on the sorted routes: util.rowwise_adagrad_segments_f64 over the
per-lookup gradient rows (weight x bag gradient) in the order the partition leaves the hits in -- behind the misses, REVERSED
(cub::DevicePartition::Flagged's rejects) -- which is the order "index order within a row" refers to.

Axes and what was pruned (E = 11,000 rows, ranks 16, one forward and one backward per module):
  lookups   10,240 (owner / atomic) | 40,960 (past the owner kernel's 32,768) | 81,920 (past Adagrad's auto switch) |
            270,336 = 8192 x 33 (past the SGD / dense auto switch)
  width     q = [4,4,4] D = 64 | q = [3,5,6] D = 90 (D % 4 != 0: the chain at every size, float columns) | q = [8,8,5] D = 320 (D > 256:
            the chain at every size)
  optimizer dense | SGD | row-wise Adagrad on the cache rows (EXACT_ADAGRAD on the cores)
  deterministic_cache_update   None | True | False
  weights   none | per_sample_weights with requires_grad | without   (negatives and exact zeros among them)
  stream    Zipf 1.2 over a cache of 200 rows (about 69 % hits) | uniform over a cache of 2000 (about 18 % hits)
Kept: D = 64, Zipf: every size x optimizer x {None, True}, unweighted and weighted-with-gradient; False at the smallest and the
largest size (at 40,960 and 81,920 it is the same atomic launch); weights without a gradient at 81,920 / None only (the flag only
adds the weights' own backward, which the weighted-with-gradient cases hold).  D = 90 and D = 320: the smallest size and 81,920
(True; None for Adagrad at 81,920; False at the smallest) -- 40,960 and 270,336 take the same chain as 81,920.  Uniform stream: 40,960 /
True, 270,336 / None, 81,920 / None for Adagrad, weighted only (the unweighted glue does not depend on the hit share).  The Python
autograd function: the auto-switch test only (it refuses weights; everything behind the switch is the same C ABI).
Edges (40,960 lookups, D = 64, True: the chain): every lookup a hit, every lookup a miss, an empty bag at each end, one cache
row taking a third of the batch.
"""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
from util import assert_close, assert_adagrad_close, rowwise_adagrad_segments_f64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

P, RANKS, E_ = [20, 22, 25], [16, 16], 11_000
LR, EPS = 0.05, 1.0e-4
SIZES = {10_240: (512, 20), 40_960: (2048, 20), 81_920: (4096, 20), 270_336: (8192, 33),
         # the auto thresholds themselves and one bag length below them (test_auto_switch_*)
         57_344: (8192, 7), 65_536: (8192, 8), 253_952: (8192, 31), 262_144: (8192, 32)}
STREAMS = {"zipf": (1.2, 200), "uniform": (1.0, 2000)}  # alpha of the request stream, cache rows
# Tolerances: the default of tests/util.py (rtol 1e-5, atol 2e-6 max|ref|) for everything -- the sorted tests of tests/test_cache_gpu.py
# allow twice that from 100,000 lookups on; it is not needed here (hottest row: 45,000 terms) -- except the row-wise Adagrad state and
# rows of the cache, which those tests hold at rtol 2e-5 / atol 4e-6 max|ref| at every size: the state is a running fp32 sum in
# another association than the reference's, and every step's size is computed from it.
ADAGRAD_TOL = dict(rtol=2e-5, atol_scale=4e-6)


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture
def routes(monkeypatch):
    """the route under test is the one the case names: nothing in the environment overrides `deterministic_cache_update=None`
    or moves the thresholds"""
    import tt_embeddings as E
    import tt_embeddings_ops as ops

    for v in ("TTX_DETERMINISTIC", "TTX_DETERMINISTIC_AUTO_MIN_NNZ", "TTX_DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD", "TTX_NO_NATIVE_NODE"):
        monkeypatch.delenv(v, raising=False)
    assert E.DETERMINISTIC_AUTO_MIN_NNZ == 262144 and E.DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD == 65536
    assert ops._native_node() is not None, "ttx_torch.so not built / not importable on this box"
    return ops


def _optimizer(ops, optim):
    return {"dense": None, "sgd": ops.OptimType.SGD, "adagrad": ops.OptimType.EXACT_ADAGRAD}[optim]


def _auto_threshold(optim):
    return 65536 if optim == "adagrad" else 262144


_LIVE = {}


def _live_module(ops, q, optim, stream, det):
    """a module whose cache went live on a warm-up stream of `stream`'s kind (built once per shape / optimizer / stream, every
    case gets a copy of that state), the keys of its cache and their rows, and the keys a request must leave out"""
    alpha, cache_size = STREAMS[stream]
    optimizer = _optimizer(ops, optim)
    kw = dict(num_embeddings=E_, embedding_dim=int(np.prod(q)), tt_ranks=RANKS, tt_p_shapes=P, tt_q_shapes=list(q),
              weight_dist="uniform", device=DEV, sparse=optimizer is not None, optimizer=optimizer or ops.OptimType.SGD,
              learning_rate=LR, eps=EPS, use_cache=True, cache_size=cache_size, hashtbl_size=1 << 20)
    key = (tuple(q), optim, stream)
    if key not in _LIVE:
        torch.manual_seed(11)
        a = ops.TTEmbeddingBag(**kw)
        with torch.no_grad():
            for i, o in G.make_requests(70, 3, 512, 1, 20, E_, alpha=alpha):
                a(t(i), t(o))
        a.cache_populate()
        if a.cache_optimizer_state is not None:
            # a state that is not all zero: the step sizes depend on it.  (The row-wise state of the cache rows is the FIRST
            # cache_size floats of the buffer, whatever its shape -- [cache_size, D] with EXACT_ADAGRAD, as in the reference.)
            a.cache_optimizer_state.view(-1)[:cache_size] = t((np.random.RandomState(3).rand(cache_size) * 0.01).astype(np.float32))
        # A CACHED key that sits behind its home slot with an empty slot in front of it gets a second seat the next time it is
        # counted and is a miss from then on (the reference's insert, hashtbl_cuda_utils.cuh:102-133; see _cache_live_pair in
        # test_module_gpu.py): the requests leave those few keys out, so that "cached" below is what the forward will see.
        keys, state = a.hashtbl.cpu().numpy(), a.cache_state.cpu().numpy()
        H = keys.size
        prone = set()
        for s_ in np.nonzero(state >= 0)[0]:
            k = int(keys[s_])
            c = O.hash64(k, H)
            while c != s_:
                if keys[c] == -1:
                    prone.add(k)
                    break
                c = (c + 1) % H
        ok = (keys >= 0) & (state >= 0) & ~np.isin(keys, list(prone))
        _LIVE[key] = ({k_: v.detach().clone() for k_, v in a.state_dict().items()}, keys[ok].copy(), state[ok].astype(np.int64),
                      np.array(sorted(prone), dtype=np.int64))
    sd, ck, crow, prone = _LIVE[key]
    torch.manual_seed(11)
    m = ops.TTEmbeddingBag(deterministic_cache_update=det, **kw)
    m.load_state_dict(sd)
    m.warmup = False
    return m, ck, crow, prone, kw


def _full_table_f64(q, cores):
    """the cores [1, p_t, r_t q_t r_t+1] (the module's storage layout) expanded to the [E, D] table, in the cores' precision"""
    r = [1] + RANKS + [1]
    acc = None
    for k, c in enumerate(cores):
        m = c.reshape(P[k], r[k], q[k], r[k + 1]).permute(1, 0, 2, 3)  # [r, p, q, r']
        acc = m.reshape(-1, r[k + 1]) if acc is None else acc.reshape(-1, r[k]) @ m.reshape(r[k], -1)
    T = len(P)
    acc = acc.reshape([d for pq in zip(P, q) for d in pq])
    return acc.permute(list(range(0, 2 * T, 2)) + list(range(1, 2 * T, 2))).reshape(int(np.prod(P)), int(np.prod(q)))


def _weights(nnz, seed):
    """per_sample_weights in [-0.5, 1.5) with exact zeros: negatives flip a lookup's gradient row, zeros erase it"""
    rs = np.random.RandomState(seed)
    w = (rs.rand(nnz) * 2 - 0.5).astype(np.float32)
    w[rs.rand(nnz) < 0.05] = 0.0
    return w


def _request(nnz, stream, prone, ck, edge=None):
    """-> indices, offsets (include_last_offset form)"""
    B, L = SIZES[nnz]
    alpha = STREAMS[stream][0]
    idx, off = G.make_requests(71, 1, B, 1, L, E_, alpha=alpha)[0]
    rs = np.random.RandomState(5)
    miss_keys = np.setdiff1d(np.arange(E_), np.concatenate([ck, prone]))
    if prone.size:
        idx = np.where(np.isin(idx, prone), miss_keys[0], idx)
    if edge == "all-hit":
        idx = ck[rs.randint(0, ck.size, size=idx.size)]
    elif edge == "all-miss":
        idx = miss_keys[rs.randint(0, miss_keys.size, size=idx.size)]
    elif edge == "hot-row":
        idx = idx.copy()
        idx[rs.permutation(idx.size)[: idx.size // 3]] = ck[ck.size // 2]
    elif edge == "empty-bags":  # the first and the last bag hold nothing (their lookups go to their neighbours)
        off = off.copy()
        off[1] = 0
        off[-2] = off[-1]
    return idx.astype(np.int64), off


class _Case:
    """one forward + backward of a live module and the float64 reference of the same step"""

    def __init__(self, ops, q, optim, det, weights, stream, nnz, edge=None, node="native", with_reference=True):
        self.optim, self.nnz, self.q, self.D = optim, nnz, q, int(np.prod(q))
        m, ck, crow, prone, self.kw = _live_module(ops, q, optim, stream, det)
        self.m = m
        idx_h, off_h = _request(nnz, stream, prone, ck, edge)
        assert idx_h.size == nnz
        B = off_h.size - 1
        self.idx, self.off = t(idx_h), t(off_h)
        row_of_key = np.full(E_, -1, dtype=np.int64)
        row_of_key[ck] = crow
        self.hit = row_of_key[idx_h] >= 0
        self.share = float(self.hit.mean())
        self.psw_h = None if weights == "none" else _weights(nnz, 4)
        self.d_out = t(G.make_grad(9, 1, B, self.D)[0])  # [B, D]
        self.cores0 = [c.detach().clone() for c in m.tt_cores]
        self.cw0 = m.cache_weight.detach().clone()
        self.cst0 = None if m.cache_optimizer_state is None else m.cache_optimizer_state.detach().clone()
        # ---- the module
        self.w = None
        if self.psw_h is not None:
            self.w = t(self.psw_h)
            if weights == "grad":
                self.w.requires_grad_(True)
        self.out = m(self.idx, self.off) if self.w is None else m(self.idx, self.off, per_sample_weights=self.w)
        self.out.backward(self.d_out)
        torch.cuda.synchronize()
        if not with_reference:
            return
        # ---- float64: the table the module served, as a function of the cores and the cache rows
        self.ref_cores = [c.double().requires_grad_(True) for c in self.cores0]
        self.ref_cw = self.cw0.double().requires_grad_(True)
        table = _full_table_f64(q, self.ref_cores).index_put((t(ck),), self.ref_cw[t(crow)])
        self.w_ref = None if self.psw_h is None else t(self.psw_h).double().requires_grad_(True)
        self.ref = torch.nn.functional.embedding_bag(self.idx, table, self.off, mode="sum", per_sample_weights=self.w_ref,
                                                     include_last_offset=True)
        self.ref.backward(self.d_out.double())
        # every cached lookup's own gradient row, in the order the partition leaves the hits in (reversed), and its cache row
        pos = np.nonzero(self.hit)[0][::-1]
        bag = np.searchsorted(off_h, pos, side="right") - 1
        g = self.d_out.double().cpu().numpy()[bag]
        if self.psw_h is not None:
            g = g * self.psw_h[pos].astype(np.float64)[:, None]
        self.lookup_rows, self.lookup_loc = g, row_of_key[idx_h[pos]]
        self.touched = np.zeros(self.cw0.size(0), dtype=bool)
        self.touched[self.lookup_loc[np.abs(g).sum(axis=1) > 0]] = True

    def state(self):
        """what a step leaves behind, for bit comparisons: cache rows (dense: their gradient), cache optimizer state, cores (dense:
        their gradients)"""
        m = self.m
        if self.optim == "dense":
            return [m.cache_weight.grad.detach().clone()] + [c.grad.detach().clone() for c in m.tt_cores]
        st = [] if m.cache_optimizer_state is None else [m.cache_optimizer_state.detach().clone()]
        return [m.cache_weight.detach().clone()] + st + [c.detach().clone() for c in m.tt_cores]

    def check(self, sorted_route):
        m, optim = self.m, self.optim
        tag = f"{optim} nnz={self.nnz} D={self.D} hit share {self.share:.3f}: "
        assert_close(self.out.detach().cpu().numpy(), self.ref.detach().cpu().numpy(), tag + "forward")
        if self.w is not None and self.w.requires_grad:
            assert self.w.grad is not None
            assert_close(self.w.grad.cpu().numpy(), self.w_ref.grad.cpu().numpy(), tag + "gradient of per_sample_weights")
        ref_cg = [c.grad if c.grad is not None else torch.zeros_like(c) for c in self.ref_cores]
        ref_cwg = self.ref_cw.grad if self.ref_cw.grad is not None else torch.zeros_like(self.ref_cw)
        untouched = t(~self.touched)
        if optim == "dense":
            for k in range(3):
                assert_close(m.tt_cores[k].grad.cpu().numpy(), ref_cg[k].cpu().numpy(), tag + f"core {k} gradient (misses)")
            got = m.cache_weight.grad
            assert_close(got.cpu().numpy(), ref_cwg.cpu().numpy(), tag + "cache row gradient (hits)")
            assert not bool(got[untouched].any()), "dense: the gradient of rows nobody hit must be exactly zero"
            return
        got = m.cache_weight.detach()
        assert torch.equal(got[untouched], self.cw0[untouched]), "rows nobody hit must not change by a bit"
        if optim == "sgd":
            for k in range(3):
                assert_close(m.tt_cores[k].detach().cpu().numpy(), (self.cores0[k].double() - LR * ref_cg[k]).cpu().numpy(),
                             tag + f"core {k} after SGD")
            assert_close(got.cpu().numpy(), (self.cw0.double() - LR * ref_cwg).cpu().numpy(), tag + "cache rows after SGD")
            return
        # Adagrad.  Cores (element-wise, first step from a zero state): w - lr g / (sqrt(g^2) + eps)
        for k in range(3):
            g = ref_cg[k].cpu().numpy()
            assert_adagrad_close(m.tt_cores[k].detach().cpu().numpy(), self.cores0[k].double().cpu().numpy() - LR * g / (np.abs(g) + EPS),
                                 g, tag + f"core {k} after Adagrad", lr=LR, eps=EPS)
        cs = self.cw0.size(0)
        assert torch.equal(m.cache_optimizer_state.detach().reshape(-1)[cs:], self.cst0.reshape(-1)[cs:]), \
            "the buffer behind the row-wise state must not be written"
        st_got, st0 = m.cache_optimizer_state.detach().reshape(-1)[:cs], self.cst0.reshape(-1)[:cs]
        assert torch.equal(st_got[untouched], st0[untouched]), "the state of rows nobody hit must not change by a bit"
        st64, w64 = rowwise_adagrad_segments_f64(self.lookup_rows, self.lookup_loc, np.arange(self.lookup_loc.size), LR, EPS,
                                                 st0.cpu().numpy(), self.cw0.cpu().numpy())
        # (the state totals do not depend on the order: both routes)
        assert_close(st_got.cpu().numpy(), st64, tag + "cache optimizer state", **ADAGRAD_TOL)
        if sorted_route:  # index order within a row is the defined order: the values, at any size
            assert_close(got.cpu().numpy(), w64, tag + "cache rows after row-wise Adagrad", **ADAGRAD_TOL)
        else:  # atomic: the `old` a lookup sees depends on arrival order, as in the reference -- which rows moved
            assert bool(torch.isfinite(got).all())
            moved = ((got - self.cw0).abs().sum(dim=1) > 0).cpu().numpy()
            assert np.array_equal(moved, self.touched), "exactly the rows that were hit by a non-zero gradient row move"


def _assert_both_parts(case):
    n_hit = int(case.hit.sum())
    assert 0 < n_hit < case.nnz, "the batch must hold hits and misses"
    assert 0.05 <= case.share <= 0.95, f"degenerate stream: hit share {case.share:.3f}"


def _assert_real_split(case):
    """the module's own hash table agrees with the reference's idea of what is cached (no counting: frequencies stay)"""
    import tt_embeddings as E

    n_tt = E.preprocess_indices_sync(case.idx, case.off, 1, False, case.m.hashtbl, case.m.cache_state)[3]
    assert int(n_tt) == case.nnz - int(case.hit.sum()), "the module's split point is not the reference's miss count"


def _grid():
    out = []
    for nnz in (10_240, 40_960, 81_920, 270_336):
        for optim in ("dense", "sgd", "adagrad"):
            for det in (None, True):
                out += [((4, 4, 4), nnz, optim, det, "none", "zipf"), ((4, 4, 4), nnz, optim, det, "grad", "zipf")]
            if nnz in (10_240, 270_336):
                out += [((4, 4, 4), nnz, optim, False, "none", "zipf"), ((4, 4, 4), nnz, optim, False, "grad", "zipf")]
    for optim in ("dense", "sgd", "adagrad"):
        out.append(((4, 4, 4), 81_920, optim, None, "nograd", "zipf"))
        for q in ((3, 5, 6), (8, 8, 5)):
            out += [(q, 10_240, optim, True, "grad", "zipf"), (q, 81_920, optim, True, "none", "zipf"),
                    (q, 10_240, optim, False, "none", "zipf")]
        out += [((4, 4, 4), 40_960, optim, True, "grad", "uniform"), ((4, 4, 4), 270_336, optim, None, "grad", "uniform")]
    for q in ((3, 5, 6), (8, 8, 5)):
        out.append((q, 81_920, "adagrad", None, "grad", "zipf"))
    out.append(((4, 4, 4), 81_920, "adagrad", None, "grad", "uniform"))
    return out


def _id(c):
    q, nnz, optim, det, weights, stream = c
    return f"D{int(np.prod(q))}-{nnz}-{optim}-det{det}-w{weights}-{stream}"


@pytest.mark.parametrize("case", _grid(), ids=_id)
def test_cache_live_step_across_the_routes(routes, case):
    """forward, the gradient of the weights, the cores and the cache rows of one cache-live training step against float64; rows
    nobody hit stay bit for bit; on the sorted routes a second module run from the same state leaves the same bits"""
    q, nnz, optim, det, weights, stream = case
    sorted_route = det is True or (det is None and nnz >= _auto_threshold(optim))
    c = _Case(routes, q, optim, det, weights, stream, nnz)
    _assert_both_parts(c)
    _assert_real_split(c)
    c.check(sorted_route)
    if sorted_route:
        again = _Case(routes, q, optim, det, weights, stream, nnz, with_reference=False)
        for x, y in zip(c.state(), again.state()):
            assert torch.equal(x, y), "two runs from the same state must be bit-identical on the sorted routes"


@pytest.mark.parametrize("edge", ["all-hit", "all-miss", "empty-bags", "hot-row"])
@pytest.mark.parametrize("optim", ["dense", "sgd", "adagrad"])
def test_sort_chain_edges_through_the_module(routes, optim, edge):
    """40,960 weighted lookups, D = 64, deterministic: the sort chain.  Every lookup a hit (split point 0); every lookup a miss
    (split point = nnz: the cache rows -- Adagrad: and the cache state -- bit-unchanged, the dense cache gradient all zero); an
    empty bag at each end; one cache row taking a third of the batch (a run that spans a thousand slices)."""
    c = _Case(routes, (4, 4, 4), optim, True, "grad", "zipf", 40_960, edge=edge)
    n_hit = int(c.hit.sum())
    if edge == "all-hit":
        assert n_hit == c.nnz
    elif edge == "all-miss":
        assert n_hit == 0
    else:
        _assert_both_parts(c)
    if edge == "hot-row":
        assert np.bincount(c.lookup_loc).max() >= c.nnz // 3
    _assert_real_split(c)
    c.check(True)
    if edge == "all-miss":
        if optim == "dense":
            assert not bool(c.m.cache_weight.grad.any())
        else:
            assert torch.equal(c.m.cache_weight.detach(), c.cw0)
            if optim == "adagrad":
                assert torch.equal(c.m.cache_optimizer_state.detach(), c.cst0)
    again = _Case(routes, (4, 4, 4), optim, True, "grad", "zipf", 40_960, edge=edge, with_reference=False)
    for x, y in zip(c.state(), again.state()):
        assert torch.equal(x, y)


@pytest.mark.parametrize("optim", ["dense", "sgd", "adagrad"])
@pytest.mark.parametrize("node,weights", [("native", "none"), ("native", "grad"), ("python", "none")])  # (the Python function takes no weights)
def test_auto_switch_of_the_cache_update(routes, monkeypatch, node, optim, weights):
    """`deterministic_cache_update=None` switches to the sorted update at 65,536 lookups PER BATCH (row-wise Adagrad) / 262,144
    (SGD, dense) -- misses and hits together, on both autograd routes (the C++ node keeps the split point on
    the device, the Python function follows it).  AT the threshold None equals True bit for bit -- cache rows, cache state, cores --
    and two None runs equal each other; one bag length below it None is the atomic update: equal to False to tolerance (float
    atomics: not to the bit; row-wise Adagrad's rows, whose step sizes depend on the arrival order on that route as in the
    reference, are held to which rows moved, and its state to tolerance)."""
    ops = routes
    if node == "python":
        monkeypatch.setenv("TTX_NO_NATIVE_NODE", "1")
        assert ops._native_node() is None
    thr = _auto_threshold(optim)
    below = {65536: 57_344, 262144: 253_952}[thr]
    q = (4, 4, 4)
    run = lambda det, nnz: _Case(ops, q, optim, det, weights, "zipf", nnz, with_reference=False)  # noqa: E731
    auto, forced, auto2 = run(None, thr), run(True, thr), run(None, thr)
    _assert_both_parts(auto)
    for x, y, z in zip(auto.state(), forced.state(), auto2.state()):
        assert torch.equal(x, y), f"None must take the sorted update from {thr} lookups on"
        assert torch.equal(x, z), "two runs of the auto-selected sorted update differ"
    auto, atomic = run(None, below), run(False, below)
    _assert_both_parts(auto)
    names = (["cache row gradient"] if optim == "dense" else ["cache rows"] + (["cache state"] if optim == "adagrad" else [])) + \
        ["core 0", "core 1", "core 2"]
    for what, x, y in zip(names, auto.state(), atomic.state()):
        if optim == "adagrad" and what == "cache rows":
            assert torch.equal((x != auto.cw0).any(dim=1), (y != atomic.cw0).any(dim=1)), "None and False moved different rows"
            continue
        if optim == "adagrad" and what.startswith("core"):
            # (the cores' element-wise Adagrad step does not depend on the cache route at all: the same kernels, the same bits)
            assert torch.equal(x, y), f"{what}: the cores' step must not depend on the cache route"
            continue
        assert_close(x.cpu().numpy(), y.cpu().numpy(), f"{below} lookups, {what}: None vs False",
                     **(ADAGRAD_TOL if what == "cache state" else {}))
