"""GPU tests of the row cache over several tables, `TableBatchedTTEmbeddingBag(num_tables > 1, use_cache=True)`:
the kernels table_keys / table_keys_split / cache_populate_tables against numpy (integers exactly, cache rows against the float64
rows), and the module -- warm-up counting of keys, the live forward against an uncached twin with the same cores (and, with a
known perturbation of the cache rows, against the twin plus the perturbation of the HOST's hit map), one fused SGD / row-wise
Adagrad / dense step with the cores against the twin stepped on the misses only and the cache rows against float64 restatements,
mean pooling, eviction, the edges, and capture.

Every module stream holds a table with only hits (table 0), a table with only misses (table 1, which also looks up the local
indices that are hot in table 0: the aliasing case), a mixed table (2), and empty bags."""
import collections

import numpy as np
import pytest
import torch

import gen_inputs as G
import tt_ref64 as R64
from test_pooling_modes_gpu import t
from util import EPS, LR, assert_adagrad_close, assert_close, rowwise_adagrad_segments_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT, B = 3, 8
GEOMS = [("generic", [5, 6, 7], [3, 3, 5], [6, 7]), ("spec", [200, 220, 250], [4, 4, 4], [32, 32])]
GEOM_IDS = [g[0] for g in GEOMS]
SENT = -777


def stream():
    return torch.cuda.current_stream().cuda_stream


def test_the_two_geometries_take_the_two_kernel_families():
    import tt_embeddings as E

    for name, p, q, r in GEOMS:
        mc = E.debug_tiles(NT, p, q, [1] + r + [1])["MC"]
        assert (mc != 0) == (name == "generic"), (name, mc)  # (0: a shape-specialised kernel takes the geometry)


# ------------------------------------------------------------------------------------------------------------------ kernels
def np_bags(nt, Bk, nnz, seed):
    """nt * Bk bags holding nnz lookups: about a third of the bags empty, and (nt >= 3) table 1 without any lookup"""
    rs = np.random.RandomState(seed)
    w = rs.rand(nt * Bk) * (rs.rand(nt * Bk) > 0.3)
    if nt >= 3:
        w[Bk:2 * Bk] = 0
    if w.sum() == 0:
        w[0] = 1
    lens = rs.multinomial(nnz, w / w.sum())
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bag = np.repeat(np.arange(nt * Bk, dtype=np.int64), lens)
    return off, bag


@pytest.mark.parametrize("nt", [1, 3, 64, 200, 1100])  # (1100: more table boundaries than are staged in LDS)
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, 70000])
def test_table_keys_vs_numpy(nt, nnz):
    import tt_embeddings as E

    Bk, stride = 3, 1 << 33  # (a stride beyond 2^32: 32-bit arithmetic anywhere would truncate)
    off, bag = np_bags(nt, Bk, nnz, nt + nnz)
    idx = np.random.RandomState(nnz).randint(0, stride, size=nnz, dtype=np.int64)
    want = idx + (bag // Bk) * stride
    if nt >= 3:
        assert not ((bag // Bk) == 1).any() and off[Bk] == off[2 * Bk], "a table with no lookups"
        assert (np.diff(off) == 0).any(), "empty bags"
    got = E.table_keys(t(idx), t(off), nt, stride).cpu().numpy()
    assert np.array_equal(got, want)
    if (bag // Bk).max() >= 1:
        assert int(want.max()) >= 1 << 33


def table_map(ht, fr):
    ht, fr = ht.cpu().numpy(), fr.cpu().numpy()
    return {int(k): int(v) for k, v in zip(ht[ht >= 0], fr[ht >= 0])}


def test_table_keys_counts_what_it_forms():
    import tt_embeddings as E

    nt, Bk, nnz, stride, H = 3, 5, 5000, 1 << 33, 4096
    off, bag = np_bags(nt, Bk, nnz, 77)
    idx = np.random.RandomState(78).zipf(1.3, size=nnz).astype(np.int64) % 150
    keys = idx + (bag // Bk) * stride
    want = collections.Counter(keys.tolist())
    assert H >= 8 * len(want)
    ht = torch.full((H,), -1, dtype=torch.int64, device=DEV)
    fr = torch.zeros(H, dtype=torch.int64, device=DEV)
    got_keys = E.table_keys(t(idx), t(off), nt, stride, ht, fr).cpu().numpy()
    assert np.array_equal(got_keys, keys)
    got = table_map(ht, fr)
    assert sum(got.values()) == nnz, "precondition: no key ran out of its three probes"
    assert got == dict(want)
    # ... and exactly what update_cache_state leaves on the same keys (the same slots: the hash sees the same keys)
    ht2, fr2 = torch.full_like(ht, -1), torch.zeros_like(fr)
    E.update_cache_state(t(keys), ht2, fr2)
    assert table_map(ht2, fr2) == got


def raw_split(keys, bagrow, nt, Bk, stride, n_dev):
    """through the C ABI into sentinel-filled outputs -> (indices, tableidx, rowidx)"""
    import tt_embeddings as E

    lib = E.lib()
    n = keys.size
    k, b = t(keys), None if bagrow is None else t(bagrow)
    outs = [torch.full((n,), SENT, dtype=torch.int64, device=DEV) for _ in range(3)]
    cnt = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    rc = lib.ttx_table_keys_split(n, None if cnt is None else cnt.data_ptr(), nt, Bk, stride, k.data_ptr(),
                                  None if b is None else b.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                  stream())
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_table_keys_split_is_the_inverse(n):
    import tt_embeddings as E

    nt, Bk, stride = 7, 4, 1 << 33
    off, bag = np_bags(nt, Bk, n, n + 1)
    rs = np.random.RandomState(n)
    idx = rs.randint(0, stride, size=n, dtype=np.int64)
    perm = rs.permutation(n)  # (a partitioned batch is not table-major any more)
    idx, bag = idx[perm], bag[perm]
    keys = t(idx + (bag // Bk) * stride)
    got = E.table_keys_split(keys, t(bag), nt, Bk, stride)
    for g, w, what in zip(got, (idx, bag // Bk, bag % Bk), ("indices", "tableidx", "rowidx")):
        assert np.array_equal(g.cpu().numpy(), w), what
    knp = keys.cpu().numpy()
    for n_dev in (None, n // 3, n, n + 50, -5):
        cnt = n if n_dev is None else min(max(n_dev, 0), n)
        gi, gt, gr = raw_split(knp, bag, nt, Bk, stride, n_dev)
        assert np.array_equal(gi[:cnt], idx[:cnt]) and np.array_equal(gt[:cnt], (bag // Bk)[:cnt]) and np.array_equal(gr[:cnt], (bag % Bk)[:cnt])
        assert (gi[cnt:] == SENT).all() and (gt[cnt:] == SENT).all() and (gr[cnt:] == SENT).all(), "entries at and beyond the count stay"
        gi, gt, gr = raw_split(knp, None, nt, Bk, stride, n_dev)  # bagrow == NULL: the table from the key, no bag rows
        assert np.array_equal(gi[:cnt], idx[:cnt]) and np.array_equal(gt[:cnt], (bag // Bk)[:cnt])
        assert (gi[cnt:] == SENT).all() and (gt[cnt:] == SENT).all() and (gr == SENT).all()
    i2, t2, r2 = E.table_keys_split(keys, None, nt, Bk, stride)
    assert r2 is None and np.array_equal(i2.cpu().numpy(), idx) and np.array_equal(t2.cpu().numpy(), bag // Bk)


def test_table_keys_split_clamps_the_table():
    """a bag row / key beyond the last table: the table is clamped before it scales anything"""
    nt, Bk, stride = 3, 4, 100
    keys = np.array([5, 2 * stride + 7, 9 * stride + 1], np.int64)
    bag = np.array([1, 2 * Bk + 3, 40], np.int64)
    gi, gt, gr = raw_split(keys, bag, nt, Bk, stride, None)
    assert gt.tolist() == [0, 2, 2] and gi.tolist() == [5, 7, 7 * stride + 1] and gr.tolist() == [1, 3, 40 - 2 * Bk]
    gi, gt, _ = raw_split(keys, None, nt, Bk, stride, None)
    assert gt.tolist() == [0, 2, 2] and gi.tolist() == [5, 7, 7 * stride + 1]


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("cs", [32, 64], ids=["evicting", "with-empty-rows"])
def test_cache_populate_tables_vs_numpy_and_float64(geom, cs):
    """a first populate from a clean table: 50 distinct keys of three tables into 32 cache rows (18 keys leave the table) or 64
    (the 14 rows left over are row 0 of table 0)"""
    import tt_embeddings as E

    _, p, q, r = geom
    D, stride, H, Bk = int(np.prod(q)), int(np.prod(p)), 1024, 4
    ranks = [1] + r + [1]
    cores = G.make_cores(31, NT, p, q, r, "signed")
    rs = np.random.RandomState(32)
    pool = np.stack([rs.randint(0, NT, size=50), rs.choice(200, size=50, replace=False)], 1)  # 50 distinct (table, index)
    pick = np.sort(rs.zipf(1.3, size=600) % 50)
    pick = np.concatenate([np.arange(50), pick])  # every key at least once
    order = np.argsort(pool[pick, 0], kind="stable")  # table-major
    tab, idx = pool[pick, 0][order], pool[pick, 1][order].astype(np.int64)
    lens = np.zeros(NT * Bk, np.int64)
    for k in range(NT):
        lens[k * Bk] = int((tab == k).sum())  # (one bag per table holds the table's lookups, the others are empty)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ht = torch.full((H,), -1, dtype=torch.int64, device=DEV)
    fr = torch.zeros(H, dtype=torch.int64, device=DEV)
    st = torch.full((H,), -1, dtype=torch.int32, device=DEV)
    E.table_keys(t(idx), t(off), NT, stride, ht, fr)
    ht0, fr0 = ht.cpu().numpy().copy(), fr.cpu().numpy().copy()
    assert (ht0 >= 0).sum() == 50 and fr0.sum() == idx.size
    cw = torch.full((cs, D), 9.0, device=DEV)
    E.cache_populate_tables(NT, p, q, ranks, [t(c) for c in cores], ht, fr, st, cw, stride)
    torch.cuda.synchronize()
    # ---- the numpy restatement: stable descending order of the frequencies, the top cs non-empty slots ranked, the rest emptied
    order = np.argsort(-fr0, kind="stable")
    want_ht, want_fr, want_st = ht0.copy(), fr0.copy(), np.full(H, -1, np.int32)
    row_key = np.zeros(cs, np.int64)  # (an empty slot among the first cs: key 0)
    for n, slot in enumerate(order):
        if ht0[slot] == -1:
            continue
        if n < cs:
            want_st[slot] = n
            row_key[n] = ht0[slot]
        else:
            want_ht[slot], want_fr[slot] = -1, 0
    assert np.array_equal(ht.cpu().numpy(), want_ht) and np.array_equal(fr.cpu().numpy(), want_fr)
    assert np.array_equal(st.cpu().numpy(), want_st)
    assert int((want_st >= 0).sum()) == min(cs, 50)
    # ---- the cache rows: float64 rows of (key // stride, key % stride)
    rt, ri = row_key // stride, row_key % stride
    assert set(rt.tolist()) == {0, 1, 2}
    ref = R64.forward_backward(NT, p, q, r, cs, ri, np.arange(cs, dtype=np.int64), rt, cores)["out"]
    assert_close(cw.cpu().numpy(), ref[rt, np.arange(cs)], f"{geom[0]} cache rows of {cs}")


# ------------------------------------------------------------------------------------------------------------------- module
HOT0 = np.arange(10, 50, dtype=np.int64)    # hot in table 0 (and looked up, cold, in tables 1 and 2: the aliasing case)
HOT2 = np.arange(100, 130, dtype=np.int64)  # hot in table 2
COLD = np.arange(150, 210, dtype=np.int64)  # never counted anywhere


def make(geom, cores, nt=NT, **kw):
    import tt_embeddings_ops as ops

    _, p, q, r = geom
    kw = dict(dict(use_cache=True, cache_size=128, hashtbl_size=4096, weight_dist="uniform", device=DEV), **kw)
    if not kw["use_cache"]:
        kw.pop("cache_size"), kw.pop("hashtbl_size"), kw.pop("deterministic_cache_update", None)
    m = ops.TableBatchedTTEmbeddingBag(nt, int(np.prod(p)), int(np.prod(q)), r, p, q, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(src if torch.is_tensor(src) else t(src))
    return m


def bag_lens(seed):
    """NT * B bags of 0 .. 5 lookups; bags 2 (table 0), B + 1 (table 1) and 2 B + 5 (table 2) empty, no table empty"""
    lens = np.random.RandomState(seed).randint(0, 6, size=NT * B)
    lens[[0, B, 2 * B]] = [4, 5, 5]
    lens[[2, B + 1, 2 * B + 5]] = 0
    return lens


def make_batch(seed, share0=1.0, share2=0.5, unique=False, lens=None, table1=True):
    """-> (indices, offsets, table per lookup, flat bag per lookup).  Table 0 draws from HOT0 with probability share0 (else COLD),
    table 1 from HOT0 and COLD (never a hit), table 2 from HOT2 with probability share2 (else HOT0[:10] and COLD).  unique: no hot
    key is drawn twice.  table1=False: table 1 has no lookups."""
    rs = np.random.RandomState(seed)
    lens = bag_lens(seed) if lens is None else np.array(lens)
    if not table1:
        lens[B:2 * B] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bag = np.repeat(np.arange(NT * B, dtype=np.int64), lens)
    tab = bag // B
    left = {0: list(rs.permutation(HOT0)), 2: list(rs.permutation(HOT2))}
    cold = {0: COLD, 1: np.concatenate([HOT0, COLD]), 2: np.concatenate([HOT0[:10], COLD])}
    idx = np.empty(bag.size, np.int64)
    for n, k in enumerate(tab):
        share = {0: share0, 1: 0.0, 2: share2}[int(k)]
        if rs.rand() < share and (not unique or left[int(k)]):
            idx[n] = left[int(k)].pop() if unique else rs.choice(HOT0 if k == 0 else HOT2)
        else:
            idx[n] = rs.choice(cold[int(k)])
    return idx, off, tab, bag


def warm_up(m):
    """two batches that count HOT0 under table 0 and HOT2 under table 2 (table 1 is never looked up while the cache warms up):
    70 keys into 128 cache rows of a 4096-slot table -- populate evicts nothing"""
    for rep0, rep2 in ((13, 7), (5, 20)):
        i0, i2 = np.concatenate([HOT0, HOT0[:rep0]]), np.concatenate([HOT2, HOT2[:rep2]])
        lens = np.zeros(NT * 2, np.int64)
        lens[[0, 1, 4, 5]] = [i0.size - 9, 9, 11, i2.size - 11]
        with torch.no_grad():
            m(t(np.concatenate([i0, i2])), t(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)))
    assert m.warmup
    m.cache_populate()
    assert not m.warmup
    return m


def cached_rows(m):
    """{key: cache row} from the module's own hash table"""
    ht, cs = m.hashtbl.cpu().numpy(), m.cache_state.cpu().numpy()
    return {int(ht[s]): int(cs[s]) for s in range(ht.size) if ht[s] >= 0 and cs[s] >= 0}


def optim_kw(optim):
    import tt_embeddings_ops as ops

    optimizer = {"dense": None, "sgd": ops.OptimType.SGD, "adagrad": ops.OptimType.EXACT_ROWWISE_ADAGRAD}[optim]
    return dict(sparse=optimizer is not None, optimizer=optimizer or ops.OptimType.SGD, learning_rate=LR, eps=EPS)


_CORES, _LIVE = {}, {}


def cores_of(geom):
    if geom[0] not in _CORES:
        _CORES[geom[0]] = G.make_cores(41, NT, geom[1], geom[2], geom[3], "signed")
    return _CORES[geom[0]]


def live_module(geom, optim="sgd", det=None, mode="sum", **extra):
    """a module whose cache is live.  The state is built once per (geometry, optimizer) and every case gets a copy (which of two
    colliding keys takes which slot of the hash table is left to arrival order: bit comparisons between two modules must not
    depend on it)."""
    key = (geom[0], optim)
    kw = optim_kw(optim)
    if key not in _LIVE:
        m = warm_up(make(geom, cores_of(geom), **kw))
        if m.cache_optimizer_state is not None:  # a state that is not all zero: the step sizes depend on it
            m.cache_optimizer_state.copy_(t((np.random.RandomState(3).rand(128) * 0.01).astype(np.float32)))
        _LIVE[key] = {k: v.detach().clone() for k, v in m.state_dict().items()}
    m = make(geom, cores_of(geom), deterministic_cache_update=det, mode=mode, **kw, **extra)
    m.load_state_dict(_LIVE[key])
    m.warmup = False
    return m


def hit_map(m, geom, idx, tab):
    """the HOST's view: which lookups are hits, and their cache rows, from (hashtbl, cache_state) and numpy keys"""
    loc_of = cached_rows(m)
    keys = idx + tab * int(np.prod(geom[1]))
    hit = np.array([int(k) in loc_of for k in keys], bool)
    loc = np.array([loc_of.get(int(k), -1) for k in keys])
    return hit, loc, loc_of


def assert_stream_shape(hit, idx, tab, off):
    assert hit[tab == 0].all() and (tab == 0).any(), "table 0: only hits"
    assert not hit[tab == 1].any() and (tab == 1).any(), "table 1: only misses"
    assert hit[tab == 2].any() and not hit[tab == 2].all(), "table 2: both"
    assert (np.diff(off) == 0).any(), "an empty bag"
    alias = np.isin(idx, HOT0) & (tab != 0)
    assert alias.any() and not hit[alias].any(), "an index that is hot in table 0 is cold in tables 1 and 2"


def misses_only(idx, off, hit):
    """the batch with the hits removed on the host"""
    keep = ~hit
    before = np.concatenate([[0], np.cumsum(keep)])
    return idx[keep], before[off].astype(np.int64)


def twin_of(m, geom, optim, mode="sum", cores=None, **extra):
    """the same module without a cache, with the cores `m` has now"""
    return make(geom, [c.detach().clone() for c in m.tt_cores] if cores is None else cores, use_cache=False, mode=mode,
                **optim_kw(optim), **extra)


def grad_of(geom, seed):
    return (np.random.RandomState(seed).rand(NT, B, int(np.prod(geom[2]))) * 0.1).astype(np.float32)


def test_warm_up_counts_keys():
    """after two batches {key: frequency} is the numpy count of the global keys (4096 slots for < 200 keys; asserted: every lookup
    is counted, no key ran out of probes)"""
    geom = GEOMS[0]
    stride = int(np.prod(geom[1]))
    m = make(geom, cores_of(geom), **optim_kw("sgd"))
    twin = twin_of(m, geom, "sgd")
    want, n = collections.Counter(), 0
    for seed in (51, 52):
        idx, off, tab, _ = make_batch(seed)
        with torch.no_grad():
            out = m(t(idx), t(off))
            assert torch.equal(out, twin(t(idx), t(off))), "counting keys changes nothing about the lookup"
        want.update((idx + tab * stride).tolist())
        n += idx.size
    got = table_map(m.hashtbl, m.cache_freq)
    assert sum(got.values()) == n and got == dict(want)
    assert m.warmup and {k // stride for k in got} == {0, 1, 2}
    m.update_cache(t(idx), t(off))  # (counts keys too)
    want.update((idx + tab * stride).tolist())
    assert table_map(m.hashtbl, m.cache_freq) == dict(want)


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_live_forward_vs_twin_and_a_known_perturbation(geom):
    D = int(np.prod(geom[2]))
    m = live_module(geom)
    assert len(cached_rows(m)) == 70, "every warm-up key has a cache row"
    twin = twin_of(m, geom, "sgd")
    idx, off, tab, bag = make_batch(61)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off)
    with torch.no_grad():
        out = m(t(idx), t(off))
        ref = twin(t(idx), t(off))
    assert out.shape == (NT, B, D)
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), f"{geom[0]} live forward vs the uncached twin")
    empty = np.nonzero(np.diff(off) == 0)[0]
    assert not out.view(NT * B, D)[t(empty)].any(), "empty bags are exact zeros"
    # a hit served as a miss (or the other way round) shows once the cache rows differ from the TT rows by a known amount
    pert = (np.random.RandomState(62).standard_normal((128, D)) * 0.5).astype(np.float32)
    with torch.no_grad():
        m.cache_weight.add_(t(pert))
        out2 = m(t(idx), t(off))
    want = ref.double().cpu().numpy().reshape(NT * B, D)
    np.add.at(want, bag[hit], pert[loc[hit]].astype(np.float64))
    assert_close(out2.cpu().numpy().reshape(NT * B, D), want, f"{geom[0]} live forward with perturbed cache rows")


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_fused_sgd_step(geom):
    D = int(np.prod(geom[2]))
    m = live_module(geom, "sgd")
    twin = twin_of(m, geom, "sgd")
    idx, off, tab, bag = make_batch(71)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off)
    d_out = grad_of(geom, 72)
    cw0 = m.cache_weight.detach().clone()
    m(t(idx), t(off)).backward(t(d_out))
    mi, mo = misses_only(idx, off, hit)
    twin(t(mi), t(mo)).backward(t(d_out))
    torch.cuda.synchronize()
    for k in range(3):
        assert_close(m.tt_cores[k].detach().cpu().numpy(), twin.tt_cores[k].detach().cpu().numpy(), f"{geom[0]} sgd core{k} vs the twin on the misses")
    assert not torch.equal(m.tt_cores[1].detach(), t(cores_of(geom)[1])), "the cores moved"
    want = cw0.double().cpu().numpy()
    np.subtract.at(want, loc[hit], LR * d_out.reshape(NT * B, D).astype(np.float64)[bag[hit]])
    assert_close(m.cache_weight.detach().cpu().numpy(), want, f"{geom[0]} cache rows after SGD")
    untouched = np.ones(128, bool)
    untouched[loc[hit]] = False
    assert torch.equal(m.cache_weight.detach()[t(untouched)], cw0[t(untouched)]), "rows nobody hit must not change by a bit"


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("det", [None, True], ids=["atomic", "sorted"])
def test_rowwise_adagrad_step(geom, det):
    """no cache row is hit from two bags (asserted), so the order in which the bags' segments arrive cannot matter and the
    float64 restatement of the reference's kernel is THE result; the cores against the twin through the Adagrad bound of
    tests/util.py (state0 = 0: |g| = sqrt(the twin's state))"""
    D = int(np.prod(geom[2]))
    m = live_module(geom, "adagrad", det=det)
    twin = twin_of(m, geom, "adagrad")
    idx, off, tab, bag = make_batch(81, unique=True)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off)
    bags_of = collections.defaultdict(set)
    for lc, b in zip(loc[hit], bag[hit]):
        bags_of[int(lc)].add(int(b))
    assert all(len(v) == 1 for v in bags_of.values()), "no cache row is hit from two bags"
    d_out = grad_of(geom, 82)
    cw0, st0 = m.cache_weight.detach().clone(), m.cache_optimizer_state.detach().clone()
    m(t(idx), t(off)).backward(t(d_out))
    mi, mo = misses_only(idx, off, hit)
    twin(t(mi), t(mo)).backward(t(d_out))
    torch.cuda.synchronize()
    for k in range(3):
        s_ref = twin.optimizer_state[k].cpu().numpy()
        g = np.sqrt(s_ref.astype(np.float64))
        R64.assert_state_close(m.optimizer_state[k].cpu().numpy(), s_ref, g, f"{geom[0]} adagrad state{k} vs the twin")
        assert_adagrad_close(m.tt_cores[k].detach().cpu().numpy(), twin.tt_cores[k].detach().cpu().numpy(), g,
                             f"{geom[0]} adagrad core{k} vs the twin", lr=LR, eps=EPS)
    st64, w64 = rowwise_adagrad_segments_f64(d_out.reshape(NT * B, D), loc[hit], bag[hit], LR, EPS, st0.cpu().numpy(), cw0.cpu().numpy())
    assert_close(m.cache_optimizer_state.cpu().numpy(), st64, f"{geom[0]} cache optimizer state")
    assert_close(m.cache_weight.detach().cpu().numpy(), w64, f"{geom[0]} cache rows after row-wise Adagrad")
    untouched = np.ones(128, bool)
    untouched[loc[hit]] = False
    assert torch.equal(m.cache_weight.detach()[t(untouched)], cw0[t(untouched)])
    assert torch.equal(m.cache_optimizer_state[t(untouched)], st0[t(untouched)])


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_dense_gradients(geom):
    D = int(np.prod(geom[2]))
    m = live_module(geom, "dense")
    twin = twin_of(m, geom, "dense")
    idx, off, tab, bag = make_batch(91)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off)
    d_out = grad_of(geom, 92)
    cw0 = m.cache_weight.detach().clone()
    m(t(idx), t(off)).backward(t(d_out))
    mi, mo = misses_only(idx, off, hit)
    twin(t(mi), t(mo)).backward(t(d_out))
    torch.cuda.synchronize()
    for k in range(3):
        assert_close(m.tt_cores[k].grad.cpu().numpy(), twin.tt_cores[k].grad.cpu().numpy(), f"{geom[0]} grad{k} vs the twin on the misses")
        assert torch.equal(m.tt_cores[k].detach(), t(cores_of(geom)[k])), "dense mode leaves the cores alone"
    want = np.zeros((128, D))
    np.add.at(want, loc[hit], d_out.reshape(NT * B, D).astype(np.float64)[bag[hit]])
    assert_close(m.cache_weight.grad.cpu().numpy(), want, f"{geom[0]} cache row gradient")
    assert torch.equal(m.cache_weight.detach(), cw0)


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_mean_mode_forward(geom):
    m = live_module(geom, mode="mean")
    twin = twin_of(m, geom, "sgd", mode="mean")
    idx, off, tab, _ = make_batch(101)
    hit, _, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off)
    with torch.no_grad():
        out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), f"{geom[0]} mean forward vs the twin")
    assert (np.diff(off) > 1).any()


def test_forward_after_an_evicting_populate():
    """16 cache rows for 70 counted keys: 54 keys leave the table; whatever is served from the cache, the forward is the twin's"""
    geom = GEOMS[0]
    m = warm_up(make(geom, cores_of(geom), cache_size=16, **optim_kw("sgd")))
    assert len(cached_rows(m)) == 16 and int((m.hashtbl >= 0).sum()) == 16
    twin = twin_of(m, geom, "sgd")
    for seed in (111, 112):  # (the first batch re-inserts evicted keys: the second meets a table that has changed)
        idx, off, tab, _ = make_batch(seed)
        with torch.no_grad():
            out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
        assert_close(out.cpu().numpy(), ref.cpu().numpy(), "forward after an evicting populate")
    hit, _, _ = hit_map(m, geom, idx, tab)
    assert hit.any() and not hit[tab == 0].all()


def test_padding_idx_takes_the_read_back_route():
    """padding_idx beside a live cache over several tables: the padding is dropped on the device, the live count read back (as
    the one-table module does beside a cache), and the compacted batch takes the live route"""
    geom, pad = GEOMS[0], 5
    m = live_module(geom, padding_idx=pad)
    twin = twin_of(m, geom, "sgd", padding_idx=pad)
    idx, off, tab, _ = make_batch(151)
    idx = np.where(np.random.RandomState(152).rand(idx.size) < 0.3, pad, idx)
    hit, _, _ = hit_map(m, geom, idx, tab)
    assert (idx == pad).any() and hit.any() and not hit[idx == pad].any()
    with torch.no_grad():
        out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), "padded live forward vs the twin")
    before = m.cache_freq.sum().item()
    with torch.no_grad():
        m(t(idx), t(off))
    assert m.cache_freq.sum().item() - before == int((idx != pad).sum()), "the padding is not counted"


def snapshot(m):
    return [x.detach().clone() for x in list(m.tt_cores) + [m.cache_weight, m.cache_freq]]


@pytest.mark.parametrize("edge", ["all-hit", "all-miss", "empty"])
def test_all_hit_all_miss_and_empty_batches(edge):
    geom = GEOMS[1]
    D = int(np.prod(geom[2]))
    m = live_module(geom, "sgd", det=True)
    twin = twin_of(m, geom, "sgd")
    if edge == "empty":
        idx, off = np.zeros(0, np.int64), np.zeros(NT * B + 1, np.int64)
        tab = bag = idx
    elif edge == "all-hit":
        idx, off, tab, bag = make_batch(121, share0=1.0, share2=1.0, table1=False)  # (table 1 cannot hit: it has no lookups)
    else:
        idx, off, tab, bag = make_batch(122, share0=0.0, share2=0.0)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert hit.all() if edge == "all-hit" else not hit.any()
    before = snapshot(m)
    out = m(t(idx), t(off))
    with torch.no_grad():
        ref = twin(t(idx), t(off))
    assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), edge + " forward")
    d_out = grad_of(geom, 123)
    out.backward(t(d_out))
    torch.cuda.synchronize()
    after = snapshot(m)
    if edge == "empty":
        assert not out.any() and all(torch.equal(a, b) for a, b in zip(before, after)), "nothing moves, nothing is counted"
    elif edge == "all-hit":  # the cores do not move by a bit, the cache rows do
        assert all(torch.equal(a, b) for a, b in zip(before[:3], after[:3]))
        want = before[3].double().cpu().numpy()
        np.subtract.at(want, loc, LR * d_out.reshape(NT * B, D).astype(np.float64)[bag])
        assert_close(after[3].cpu().numpy(), want, "all-hit cache rows after SGD")
    else:  # the cache rows do not move by a bit, the cores do
        assert torch.equal(before[3], after[3])
        assert not any(torch.equal(a, b) for a, b in zip(before[:3], after[:3]))


def test_captured_step_replays_bit_identically_to_eager_steps():
    """one capture of a fused-SGD live step over static (indices, offsets, gradient); three batches with about 10 %, 60 % and 0 %
    hits copied into it between replays: the hit / miss split is not baked into the graph"""
    import ttx_graph

    geom = GEOMS[1]
    D = int(np.prod(geom[2]))
    lens = bag_lens(131)
    example = make_batch(131, lens=lens)
    batches = [make_batch(132, 0.15, 0.15, lens=lens), make_batch(133, 0.9, 0.9, lens=lens), make_batch(134, 0.0, 0.0, lens=lens)]
    g = t(grad_of(geom, 135))
    outs, shares = {False: [], True: []}, []

    def run(graphed):
        m = live_module(geom, "sgd", det=True)
        if not graphed:
            shares.extend(float(hit_map(m, geom, b[0], b[2])[0].mean()) for b in batches)
        seen = torch.zeros(NT, B, D, device=DEV)

        def step(i, o, d):
            out = m(i, o)
            seen.copy_(out.detach())
            out.backward(d)

        if graphed:
            gs = ttx_graph.GraphedStep(step, (t(example[0]), t(example[1]), g), warmup=2)
        else:
            for _ in range(2):
                step(t(example[0]), t(example[1]), g)
        for bt in batches:
            if graphed:
                gs(t(bt[0]), t(bt[1]), g)
            else:
                step(t(bt[0]), t(bt[1]), g)
            torch.cuda.synchronize()
            outs[graphed].append(seen.clone())
        return [x.detach().clone() for x in list(m.tt_cores) + [m.cache_weight]]

    eager, replayed = run(False), run(True)
    assert 0.02 < shares[0] < 0.25 and 0.4 < shares[1] < 0.8 and shares[2] == 0.0, shares
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), f"{'cache_weight' if k == 3 else f'core {k}'} differs between replay and eager"
    for a, b in zip(outs[False], outs[True]):
        assert torch.equal(a, b), "output differs between replay and eager"


def test_per_sample_weights_and_cpu_tensors_are_refused_while_live():
    geom = GEOMS[0]
    m = live_module(geom)
    idx, off, _, _ = make_batch(141)
    with pytest.raises(NotImplementedError):
        m(t(idx), t(off), per_sample_weights=torch.ones(idx.size, device=DEV))
    with pytest.raises(NotImplementedError):
        m(torch.from_numpy(idx), torch.from_numpy(off))
    with pytest.raises(NotImplementedError, match="write_back"):
        m.cache_populate(write_back=0.1)
    assert m.prefetch(t(idx), t(off)) is False
