"""GPU tests of the row cache over tables of DIFFERENT row factors, `VarTableTTEmbeddingBag(use_cache=True)` and
`MixedTTEmbeddingBag(fused=True, use_cache=True)`: the kernels table_keys_v / table_keys_split_v /
cache_populate_var_tables against numpy (integers exactly, cache rows against the float64 rows of their own tables), and the
modules -- warm-up counting of keys, the live forward against an uncached twin with the same cores (and, with a known
perturbation of the cache rows, against the twin plus the perturbation of the HOST's hit map), one fused SGD / row-wise Adagrad /
dense step with the cores against the twin stepped on the misses only and the cache rows against float64 restatements, mean
pooling, table_ranks, eviction, per-table padding, the edges, capture, and the refusals.

Every module stream holds three tables of different cardinality: one with only hits (table 0), one with only misses (table 1,
which looks up the local indices that are hot in table 0 and indices beyond table 0's cardinality), a mixed one (2), and empty
bags.  The thread block of the key kernels is 256: the sizes are the ones at which a bound or a search can go wrong."""
import collections

import numpy as np
import pytest
import torch

import gen_inputs as G
import tt_ref64 as R64
from test_pooling_modes_gpu import t
from test_table_cache_gpu import (SENT, bag_lens, cached_rows, grad_of, misses_only, np_bags, optim_kw, snapshot, stream, table_map,
                                  warm_up)
from util import EPS, LR, assert_adagrad_close, assert_close, rowwise_adagrad_segments_f64

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NT, B = 3, 8
# (name, per-table row factors, q, ranks, cardinalities): table 0 is the smallest, so table 1 has rows beyond it
GEOMS = [("generic", [[3, 4, 5], [5, 6, 7], [5, 5, 6]], [3, 3, 5], [6, 7], [58, 205, 150]),
         ("spec", [[3, 4, 5], [20, 22, 25], [5, 5, 6]], [4, 4, 4], [32, 32], [58, 10000, 150])]
GEOM_IDS = [g[0] for g in GEOMS]


def bases_of(ps):
    return np.concatenate([[0], np.cumsum([int(np.prod(np.asarray(p, dtype=np.int64))) for p in ps])]).astype(np.int64)


def test_the_two_geometries_take_the_two_kernel_families():
    import tt_embeddings as E

    for name, ps, q, r, _ in GEOMS:
        mc = E.debug_tiles(NT, ps, q, [1] + r + [1])["MC"]
        assert (mc != 0) == (name == "generic"), (name, mc)  # (0: a shape-specialised kernel takes the geometry)


# ------------------------------------------------------------------------------------------------------------------ kernels
def strides_of(nt):
    """one stride above 2^32 (32-bit arithmetic anywhere would truncate), an ordinary one, one of 1 -- over and over"""
    return [[1 << 33, 97, 1][k % 3] for k in range(nt)]


def key_space(nt):
    strides = np.asarray(strides_of(nt), np.int64)
    return strides, np.concatenate([[0], np.cumsum(strides)]).astype(np.int64)


@pytest.mark.parametrize("nt", [1, 3, 64])
@pytest.mark.parametrize("nnz", [1, 255, 256, 257, 70000])
def test_table_keys_v_vs_numpy(nt, nnz):
    import tt_embeddings as E

    Bk = 3
    strides, base = key_space(nt)
    off, bag = np_bags(nt, Bk, nnz, nt + nnz)
    tab = bag // Bk
    idx = (np.random.RandomState(nnz).randint(0, 1 << 62, size=nnz, dtype=np.int64) % strides[tab]).astype(np.int64)
    assert int(strides.max()) > 1 << 32
    if nt >= 3:
        assert (strides == 1).any() and not (tab == 1).any() and off[Bk] == off[2 * Bk], "a stride of 1; a table with no lookups"
        assert (np.diff(off) == 0).mean() > 0.2, "about a third of the bags are empty"
    want = idx + base[tab]
    got = E.table_keys(t(idx), t(off), nt, base.tolist()).cpu().numpy()
    assert np.array_equal(got, want)
    assert tab.max() == 0 or int(want.max()) >= 1 << 33


def test_table_keys_v_counts_what_it_forms():
    import tt_embeddings as E

    nt, Bk, nnz, H = 3, 5, 5000, 4096
    base = np.asarray([0, 1 << 33, (1 << 33) + 1, (1 << 33) + 301], np.int64)  # strides 2^33, 1, 300
    off, bag = np_bags(nt, Bk, nnz, 77)
    tab = bag // Bk
    assert set(tab.tolist()) == {0, 2}
    idx = np.random.RandomState(78).zipf(1.3, size=nnz).astype(np.int64) % 150
    keys = idx + base[tab]
    want = collections.Counter(keys.tolist())
    assert H >= 8 * len(want)
    ht = torch.full((H,), -1, dtype=torch.int64, device=DEV)
    fr = torch.zeros(H, dtype=torch.int64, device=DEV)
    got_keys = E.table_keys(t(idx), t(off), nt, base.tolist(), ht, fr).cpu().numpy()
    assert np.array_equal(got_keys, keys)
    got = table_map(ht, fr)
    assert sum(got.values()) == nnz, "precondition: no key ran out of its three probes"
    assert got == dict(want)
    # ... and exactly what update_cache_state leaves on the same keys (the same slots: the hash sees the same keys)
    ht2, fr2 = torch.full_like(ht, -1), torch.zeros_like(fr)
    E.update_cache_state(t(keys), ht2, fr2)
    assert table_map(ht2, fr2) == got


def raw_split(keys, bagrow, nt, Bk, base, n_dev):
    """through the C ABI into sentinel-filled outputs -> (indices, tableidx, rowidx)"""
    import ctypes

    import tt_embeddings as E

    lib = E.lib()
    n = keys.size
    k, b = t(keys), None if bagrow is None else t(bagrow)
    outs = [torch.full((n,), SENT, dtype=torch.int64, device=DEV) for _ in range(3)]
    cnt = None if n_dev is None else torch.tensor([n_dev], dtype=torch.int32, device=DEV)
    kb = (ctypes.c_int64 * (nt + 1))(*[int(v) for v in base])
    rc = lib.ttx_table_keys_split_v(n, None if cnt is None else cnt.data_ptr(), nt, Bk, kb, k.data_ptr(),
                                    None if b is None else b.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                    stream())
    assert rc == 0, lib.ttx_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("n", [1, 255, 256, 257, 5000])
def test_table_keys_split_v_with_bag_rows_is_the_inverse(n):
    import tt_embeddings as E

    nt, Bk = 7, 4
    strides, base = key_space(nt)
    off, bag = np_bags(nt, Bk, n, n + 1)
    rs = np.random.RandomState(n)
    idx = (rs.randint(0, 1 << 62, size=n, dtype=np.int64) % strides[bag // Bk]).astype(np.int64)
    perm = rs.permutation(n)  # (a partitioned batch is not table-major any more)
    idx, bag = idx[perm], bag[perm]
    tab = bag // Bk
    keys = idx + base[tab]
    got = E.table_keys_split(t(keys), t(bag), nt, Bk, base.tolist())
    for g, w, what in zip(got, (idx, tab, bag % Bk), ("indices", "tableidx", "rowidx")):
        assert np.array_equal(g.cpu().numpy(), w), what
    for n_dev in (None, -5, 0, n // 3, n, n + 7):
        cnt = n if n_dev is None else min(max(n_dev, 0), n)
        gi, gt, gr = raw_split(keys, bag, nt, Bk, base, n_dev)
        assert np.array_equal(gi[:cnt], idx[:cnt]) and np.array_equal(gt[:cnt], tab[:cnt]) and np.array_equal(gr[:cnt], (bag % Bk)[:cnt])
        assert (gi[cnt:] == SENT).all() and (gt[cnt:] == SENT).all() and (gr[cnt:] == SENT).all(), "entries at and beyond the count stay"


def test_table_keys_split_v_clamps_the_table_of_a_bag_row():
    """a bag row beyond the last table (or below the first): the table is clamped before it indexes anything"""
    nt, Bk = 3, 4
    base = np.asarray([0, 100, 101, 350], np.int64)
    keys = np.array([5, 101 + 7, 900, 3], np.int64)
    bag = np.array([1, 2 * Bk + 3, 40, -9], np.int64)
    gi, gt, gr = raw_split(keys, bag, nt, Bk, base, None)
    assert gt.tolist() == [0, 2, 2, 0] and gi.tolist() == [5, 7, 900 - 101, 3] and gr.tolist() == [1, 3, 40 - 2 * Bk, -9]


@pytest.mark.parametrize("nt", [1, 3, 64])
def test_table_keys_split_v_without_bag_rows_searches_the_key_bases(nt):
    """every first and every last key of every table (tables of stride 1: the two are one key), and random keys in between"""
    import tt_embeddings as E

    strides, base = key_space(nt)
    rs = np.random.RandomState(nt)
    rt = rs.randint(0, nt, size=3000)
    rk = base[rt] + rs.randint(0, 1 << 62, size=3000, dtype=np.int64) % strides[rt]
    keys = np.concatenate([base[:-1], base[1:] - 1, rk]).astype(np.int64)
    keys = keys[rs.permutation(keys.size)]
    want_t = np.searchsorted(base, keys, side="right") - 1
    assert want_t.min() == 0 and want_t.max() == nt - 1 and (nt == 1 or (strides == 1).any())
    i2, t2, r2 = E.table_keys_split(t(keys), None, nt, 1, base.tolist())
    assert r2 is None and np.array_equal(t2.cpu().numpy(), want_t) and np.array_equal(i2.cpu().numpy(), keys - base[want_t])
    for n_dev in (None, keys.size // 2):
        cnt = keys.size if n_dev is None else n_dev
        gi, gt, gr = raw_split(keys, None, nt, 1, base, n_dev)
        assert np.array_equal(gt[:cnt], want_t[:cnt]) and np.array_equal(gi[:cnt], (keys - base[want_t])[:cnt])
        assert (gi[cnt:] == SENT).all() and (gt[cnt:] == SENT).all() and (gr == SENT).all(), "no bag rows are written"
    # a key beyond the key space, a negative one: the last table, the first
    gi, gt, _ = raw_split(np.array([int(base[-1]) + 5, -3], np.int64), None, nt, 1, base, None)
    assert gt.tolist() == [nt - 1, 0] and gi.tolist() == [int(base[-1]) + 5 - int(base[nt - 1]), -3]


def table_cores_np(seed, ps, q, r):
    """per table [1, p_k_t, slice] float32 cores -> (the per-table lists, the module's layout [1, sum_k p_k_t, slice])"""
    per = [G.make_cores(seed + k, 1, p, q, r, "signed") for k, p in enumerate(ps)]
    return per, [np.ascontiguousarray(np.concatenate([c[s] for c in per], axis=1)) for s in range(len(q))]


POP_GEOMS = [("generic", [[5, 6, 7], [2, 3, 4], [9, 2, 5]], [3, 3, 5], [6, 7]),
             ("spec", [[20, 22, 25], [2, 3, 4], [9, 2, 5]], [4, 4, 4], [32, 32])]


@pytest.mark.parametrize("geom", POP_GEOMS, ids=GEOM_IDS)
@pytest.mark.parametrize("cs", [32, 64], ids=["evicting", "with-empty-rows"])
def test_cache_populate_var_tables_vs_numpy_and_float64(geom, cs):
    """a first populate from a clean table: 50 distinct keys of three tables into 32 cache rows (18 keys leave the table) or 64
    (the 14 rows left over are row 0 of table 0)"""
    import tt_embeddings as E

    name, ps, q, r = geom
    D, H, Bk = int(np.prod(q)), 1024, 4
    ranks = [1] + r + [1]
    base = bases_of(ps)
    assert E.key_bases_of(ps) == base.tolist()
    assert (E.debug_tiles(NT, ps, q, ranks)["MC"] != 0) == (name == "generic")
    per, cores = table_cores_np(31, ps, q, r)
    rs = np.random.RandomState(32)
    pairs = set()
    while len(pairs) < 50:
        k = int(rs.randint(0, NT))
        pairs.add((k, int(rs.randint(0, min(200, base[k + 1] - base[k])))))
    pool = np.asarray(sorted(pairs))[rs.permutation(50)]
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
    E.table_keys(t(idx), t(off), NT, base.tolist(), ht, fr)
    ht0, fr0 = ht.cpu().numpy().copy(), fr.cpu().numpy().copy()
    assert (ht0 >= 0).sum() == 50 and fr0.sum() == idx.size
    cw = torch.full((cs, D), 9.0, device=DEV)
    E.cache_populate_var_tables(ps, q, ranks, [t(c) for c in cores], ht, fr, st, cw)
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
    # ---- the cache rows: every one the float64 row of ITS OWN table
    rt = np.searchsorted(base, row_key, side="right") - 1
    ri = row_key - base[rt]
    assert set(rt.tolist()) == {0, 1, 2}
    ref = np.zeros((cs, D))
    for k in range(NT):
        rows = np.flatnonzero(rt == k)
        out = R64.forward_backward(1, ps[k], q, r, rows.size, ri[rows], np.arange(rows.size, dtype=np.int64),
                                   np.zeros(rows.size, np.int64), per[k])["out"]
        ref[rows] = out[0]
    assert_close(cw.cpu().numpy(), ref, f"{name} cache rows of {cs}")


# ------------------------------------------------------------------------------------------------------------------- module
HOT0 = np.arange(10, 50, dtype=np.int64)     # hot in table 0 (and looked up, cold, in tables 1 and 2: the aliasing case)
HOT2 = np.arange(100, 130, dtype=np.int64)   # hot in table 2
COLD0 = np.arange(50, 58, dtype=np.int64)    # never counted anywhere
COLD1 = np.arange(60, 205, dtype=np.int64)   # ... rows table 0 does not have
COLD2 = np.arange(130, 150, dtype=np.int64)


def make(geom, cores, **kw):
    import ttx_mixed

    _, ps, q, r, Es = geom
    kw = dict(dict(use_cache=True, cache_size=128, hashtbl_size=4096, weight_dist="uniform", device=DEV), **kw)
    if not kw["use_cache"]:
        kw.pop("cache_size"), kw.pop("hashtbl_size"), kw.pop("deterministic_cache_update", None)
    m = ttx_mixed.VarTableTTEmbeddingBag(Es, int(np.prod(q)), r, ps, q, **kw)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, cores):
            dst.copy_(src if torch.is_tensor(src) else t(src))
    return m


def make_batch(seed, share0=1.0, share2=0.5, unique=False, lens=None, table1=True):
    """-> (indices, offsets, table per lookup, flat bag per lookup).  Table 0 draws from HOT0 with probability share0 (else
    COLD0), table 1 from HOT0 and COLD1 (never a hit), table 2 from HOT2 with probability share2 (else HOT0[:10] and COLD2).
    unique: no hot key is drawn twice.  table1=False: table 1 has no lookups."""
    rs = np.random.RandomState(seed)
    lens = bag_lens(seed) if lens is None else np.array(lens)
    if not table1:
        lens[B:2 * B] = 0
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    bag = np.repeat(np.arange(NT * B, dtype=np.int64), lens)
    tab = bag // B
    left = {0: list(rs.permutation(HOT0)), 2: list(rs.permutation(HOT2))}
    cold = {0: COLD0, 1: np.concatenate([HOT0, COLD1]), 2: np.concatenate([HOT0[:10], COLD2])}
    idx = np.empty(bag.size, np.int64)
    for n, k in enumerate(tab):
        share = {0: share0, 1: 0.0, 2: share2}[int(k)]
        if rs.rand() < share and (not unique or left[int(k)]):
            idx[n] = left[int(k)].pop() if unique else rs.choice(HOT0 if k == 0 else HOT2)
        else:
            idx[n] = rs.choice(cold[int(k)])
    return idx, off, tab, bag


_CORES, _LIVE = {}, {}


def cores_of(geom):
    if geom[0] not in _CORES:
        _CORES[geom[0]] = table_cores_np(41, geom[1], geom[2], geom[3])[1]
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
    keys = idx + bases_of(geom[1])[tab]
    hit = np.array([int(k) in loc_of for k in keys], bool)
    loc = np.array([loc_of.get(int(k), -1) for k in keys])
    return hit, loc, loc_of


def assert_stream_shape(hit, idx, tab, off, Es):
    assert hit[tab == 0].all() and (tab == 0).any(), "table 0: only hits"
    assert not hit[tab == 1].any() and (tab == 1).any(), "table 1: only misses"
    assert hit[tab == 2].any() and not hit[tab == 2].all(), "table 2: both"
    assert (np.diff(off) == 0).any(), "an empty bag"
    alias = np.isin(idx, HOT0) & (tab != 0)
    assert alias.any() and not hit[alias].any(), "an index that is hot in table 0 is cold in tables 1 and 2"
    assert (idx[tab == 1] >= Es[0]).any(), "table 1 looks up rows beyond table 0's cardinality"
    assert all((idx[tab == k] < Es[k]).all() for k in range(NT))


def twin_of(m, geom, optim, mode="sum", cores=None, **extra):
    """the same module without a cache, with the cores `m` has now"""
    return make(geom, [c.detach().clone() for c in m.tt_cores] if cores is None else cores, use_cache=False, mode=mode,
                **optim_kw(optim), **extra)


def test_warm_up_counts_keys():
    """after two batches {key: frequency} is the numpy count of the keys key_base[table] + index (4096 slots for < 200 keys;
    asserted: every lookup is counted, no key ran out of probes)"""
    geom = GEOMS[0]
    base = bases_of(geom[1])
    m = make(geom, cores_of(geom), **optim_kw("sgd"))
    twin = twin_of(m, geom, "sgd")
    want, n = collections.Counter(), 0
    for seed in (51, 52):
        idx, off, tab, _ = make_batch(seed)
        with torch.no_grad():
            out = m(t(idx), t(off))
            assert torch.equal(out, twin(t(idx), t(off))), "counting keys changes nothing about the lookup"
        want.update((idx + base[tab]).tolist())
        n += idx.size
    got = table_map(m.hashtbl, m.cache_freq)
    assert sum(got.values()) == n and got == dict(want)
    assert m.warmup and {int(np.searchsorted(base, k, side="right")) - 1 for k in got} == {0, 1, 2}
    m.update_cache(t(idx), t(off))  # (counts keys too)
    want.update((idx + base[tab]).tolist())
    assert table_map(m.hashtbl, m.cache_freq) == dict(want)
    m.reset_cache()
    assert table_map(m.hashtbl, m.cache_freq) == {} and m.warmup


@pytest.mark.parametrize("geom", GEOMS, ids=GEOM_IDS)
def test_live_forward_vs_twin_and_a_known_perturbation(geom):
    D = int(np.prod(geom[2]))
    m = live_module(geom)
    assert len(cached_rows(m)) == 70, "every warm-up key has a cache row"
    twin = twin_of(m, geom, "sgd")
    idx, off, tab, bag = make_batch(61)
    hit, loc, _ = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off, geom[4])
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
    assert_stream_shape(hit, idx, tab, off, geom[4])
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
    assert_stream_shape(hit, idx, tab, off, geom[4])
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
    assert_stream_shape(hit, idx, tab, off, geom[4])
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
    assert_stream_shape(hit, idx, tab, off, geom[4])
    with torch.no_grad():
        out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), f"{geom[0]} mean forward vs the twin")
    assert (np.diff(off) > 1).any()


def test_table_ranks_give_cache_rows_of_the_true_rank():
    """tables of smaller ranks ride zero-padded: the populate decompresses the padded cores, which give the rows of the true
    rank -- the live forward equals the twin's, and a cached row of table 2 equals the float64 row of its OWN-rank cores"""
    geom = GEOMS[0]
    _, ps, q, r, Es = geom
    table_ranks = [r, r, [3, 4]]
    torch.manual_seed(7)
    m = make(geom, [], table_ranks=table_ranks, **optim_kw("sgd"))  # (its own initialisation: the padding is the module's)
    twin = make(geom, [c.detach().clone() for c in m.tt_cores], use_cache=False, table_ranks=table_ranks, **optim_kw("sgd"))
    warm_up(m)
    idx, off, tab, _ = make_batch(161)
    hit, loc, loc_of = hit_map(m, geom, idx, tab)
    assert_stream_shape(hit, idx, tab, off, Es)
    with torch.no_grad():
        out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), "table_ranks live forward vs the twin")
    base = bases_of(ps)
    mine = sorted(k for k in loc_of if k >= base[2])
    assert len(mine) == 30
    small = [m.table_core(2, s).detach().cpu().numpy()[None] for s in range(3)]
    rows = R64.forward_backward(1, ps[2], q, table_ranks[2], len(mine), np.asarray(mine) - base[2], np.arange(len(mine), dtype=np.int64),
                                np.zeros(len(mine), np.int64), small)["out"][0]
    got = m.cache_weight.detach().cpu().numpy()[[loc_of[k] for k in mine]]
    assert_close(got, rows, "cache rows of the rank-[3, 4] table")


def test_forward_after_an_evicting_populate():
    """16 cache rows for 70 counted keys: 54 keys leave the table; a second populate after more batches evicts again; whatever is
    served from the cache, the forward is the twin's"""
    geom = GEOMS[0]
    m = warm_up(make(geom, cores_of(geom), cache_size=16, **optim_kw("sgd")))
    assert len(cached_rows(m)) == 16 and int((m.hashtbl >= 0).sum()) == 16
    twin = twin_of(m, geom, "sgd")
    for seed in (111, 112):  # (the first batch re-inserts evicted keys: the second meets a table that has changed)
        idx, off, tab, _ = make_batch(seed)
        with torch.no_grad():
            out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
        assert_close(out.cpu().numpy(), ref.cpu().numpy(), "forward after an evicting populate")
    assert int((m.hashtbl >= 0).sum()) > 16
    m.cache_populate()  # the second populate: evicts again, and decompresses rows of other tables than the first did
    assert len(cached_rows(m)) == 16 and int((m.hashtbl >= 0).sum()) == 16 and not m.warmup
    idx, off, tab, _ = make_batch(113)
    with torch.no_grad():
        out, ref = m(t(idx), t(off)), twin(t(idx), t(off))
    assert_close(out.cpu().numpy(), ref.cpu().numpy(), "forward after the second populate")
    hit, _, _ = hit_map(m, geom, idx, tab)
    assert hit.any() and not hit[tab == 0].all()


def test_padding_idx_takes_the_read_back_route():
    """padding_idx beside a live cache: the padding is dropped on the device, the live count read back (as on the parent), and the
    compacted batch takes the live route"""
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
    hits copied into it between replays: the hit / miss split is not baked into the graph, and the key bases travel in the kernel
    arguments (nothing is allocated or copied from the host inside the capture)"""
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


def test_a_module_of_one_table_is_served_by_the_same_routes():
    """a fused group may hold a single table: one list of row factors, key bases [0, prod(p)] -- counted, populated and served
    live like any other (the parent's one-table routes take no per-table row factors)"""
    geom = ("one", [[5, 5, 6]], GEOMS[0][2], GEOMS[0][3], [150])
    D = int(np.prod(geom[2]))
    cores = table_cores_np(43, geom[1], geom[2], geom[3])[1]
    m = make(geom, cores, cache_size=64, **optim_kw("sgd"))
    assert m._key_space() == [0, 150] and m._tables_cache()
    rs = np.random.RandomState(44)
    lens = rs.randint(0, 6, size=B)
    lens[[0, 3]] = [5, 0]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    with torch.no_grad():
        for _ in range(2):
            m(t(rs.choice(HOT2, size=int(off[-1]))), t(off))
    assert table_map(m.hashtbl, m.cache_freq) and int(m.cache_freq.sum()) == 2 * int(off[-1])
    m.cache_populate()
    twin = twin_of(m, geom, "sgd")
    idx = np.where(rs.rand(int(off[-1])) < 0.5, rs.choice(HOT2, size=int(off[-1])), rs.choice(COLD2, size=int(off[-1]))).astype(np.int64)
    loc_of = cached_rows(m)
    hit = np.array([int(k) in loc_of for k in idx], bool)
    assert hit.any() and not hit.all()
    d_out = (rs.rand(1, B, D) * 0.1).astype(np.float32)
    cw0 = m.cache_weight.detach().clone()
    out = m(t(idx), t(off))
    with torch.no_grad():
        ref = twin(t(idx), t(off))
    assert_close(out.detach().cpu().numpy(), ref.cpu().numpy(), "one table, live forward vs the twin")
    out.backward(t(d_out))
    mi, mo = misses_only(idx, off, hit)
    twin(t(mi), t(mo)).backward(t(d_out))
    torch.cuda.synchronize()
    for k in range(3):
        assert_close(m.tt_cores[k].detach().cpu().numpy(), twin.tt_cores[k].detach().cpu().numpy(), f"one table, sgd core{k}")
    bag = np.repeat(np.arange(B, dtype=np.int64), lens)
    want = cw0.double().cpu().numpy()
    np.subtract.at(want, [loc_of[int(k)] for k in idx[hit]], LR * d_out.reshape(B, D).astype(np.float64)[bag[hit]])
    assert_close(m.cache_weight.detach().cpu().numpy(), want, "one table, cache rows after SGD")


def test_what_is_refused_while_live():
    geom = GEOMS[0]
    m = live_module(geom)
    idx, off, _, _ = make_batch(141)
    with pytest.raises(NotImplementedError):
        m(t(idx), t(off), per_sample_weights=torch.ones(idx.size, device=DEV))
    with pytest.raises(NotImplementedError):
        m(torch.from_numpy(idx), torch.from_numpy(off))
    with pytest.raises(NotImplementedError, match="write_back"):
        m.cache_populate(write_back=0.1)
    assert m.prefetch(t(idx), t(off)) is False and m.prefetch_many([(t(idx), t(off))]) is False


# --------------------------------------------------------------------------------------------------------- MixedTTEmbeddingBag
MES = [58, 205, 150, 500, 90]
MPS = [[3, 4, 5], [5, 6, 7], [5, 5, 6], [8, 8, 8], [4, 5, 5]]
MQS = [[2, 2, 3], [2, 2, 3], [2, 2, 3], [3, 2, 2], [3, 2, 2]]  # two factorings of D = 12: two fused groups with pad_q=False
MR, MD, MB = [4, 3], 12, 6
MPADS = [None, 3, None, None, 7]


def mixed(**kw):
    import ttx_mixed

    torch.manual_seed(5)
    return ttx_mixed.MixedTTEmbeddingBag(MES, MD, MR, MPS, MQS, weight_dist="uniform", device=DEV, fused=True, pad_q=False,
                                         learning_rate=LR, **kw)


def dlrm_batch(seed, hot, hot_only=()):
    """per table (indices, offsets without the closing entry): table k draws from hot[k] -- and, unless k is in hot_only, from the
    rest of its rows; bag 1 is empty; the tables' padding values turn up"""
    rs = np.random.RandomState(seed)
    idx, off = [], []
    for k, e in enumerate(MES):
        lens = rs.randint(0, 5, size=MB)
        lens[1], lens[0] = 0, 3
        i = np.where(rs.rand(int(lens.sum())) < (1.0 if k in hot_only else 0.5), rs.choice(hot[k], size=int(lens.sum())),
                     rs.randint(0, e, size=int(lens.sum()))).astype(np.int64)
        if MPADS[k] is not None and k not in hot_only:
            i[0] = MPADS[k]
        idx.append(t(i))
        off.append(t(np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)))
    return idx, off


def test_mixed_module_in_dlrm_call_form():
    """two fused groups, each with its own cache, per-table padding_idx through the sentinel route: the warm-up outputs equal an
    uncached twin's bit for bit, the live outputs equal it, and after one fused SGD step both groups' cache rows have moved while
    the cores of the group whose lookups were all hits have not moved by a bit"""
    m = mixed(use_cache=True, cache_size=600, hashtbl_size=8192, padding_idx=MPADS)
    twin = mixed(padding_idx=MPADS)
    assert m.group_tables == [[0, 1, 2], [3, 4]] and all(g.use_cache for g in m.groups)
    with torch.no_grad():
        for gm, gt in zip(m.groups, twin.groups):
            for dst, src in zip(gt.tt_cores, gm.tt_cores):
                dst.copy_(src)
    hot = [np.arange(10, 30), np.arange(40, 60), np.arange(100, 120), np.arange(200, 220), np.arange(20, 40)]
    assert all(MPADS[k] is None or MPADS[k] not in hot[k] for k in range(5))
    for seed in (201, 202, 203):
        idx, off = dlrm_batch(seed, hot)
        with torch.no_grad():
            outs, refs = m(idx, off), twin(idx, off)
        for k, (o, r) in enumerate(zip(outs, refs)):  # (beside a cache the padded batch is compacted through a read-back, the
            assert o.shape == (MB, MD)                # twin's on the device: two plans of the same lookups)
            assert_close(o.cpu().numpy(), r.cpu().numpy(), f"warm-up output of table {k}")
    counted = [int(g.cache_freq.sum()) for g in m.groups]
    assert all(c > 0 for c in counted)
    m.update_cache(idx, off)
    live = [sum(int((i != (-1 if MPADS[k] is None else MPADS[k])).sum()) for k, i in enumerate(idx) if k in tables)
            for tables in m.group_tables]
    assert [int(g.cache_freq.sum()) - c for g, c in zip(m.groups, counted)] == live, "update_cache counts keys, not the padding"
    m.cache_populate()
    assert not any(g.warmup for g in m.groups)
    assert all(len(cached_rows(g)) == int((g.hashtbl >= 0).sum()) > 0 for g in m.groups), "nothing was evicted"
    # live: group 0 mixes hits and misses, group 1 (tables 3 and 4) looks up cached rows only
    for j, k in enumerate(m.group_tables[1]):  # (what table k may look up without a miss: its rows that did get a cache row)
        bases = m.groups[1]._key_space()
        hot[k] = np.asarray([key - bases[j] for key in cached_rows(m.groups[1]) if bases[j] <= key < bases[j + 1]], np.int64)
        assert hot[k].size > 5
    idx, off = dlrm_batch(204, hot, hot_only=(3, 4))
    for g, tables in enumerate(m.group_tables):
        loc_of, bases = cached_rows(m.groups[g]), m.groups[g]._key_space()
        hits = np.concatenate([[int(v) + bases[j] in loc_of for v in idx[k].cpu().numpy() if v != MPADS[k]] for j, k in enumerate(tables)])
        assert hits.all() if g == 1 else (hits.any() and not hits.all()), (g, hits.mean())
    cores0 = [[c.detach().clone() for c in g.tt_cores] for g in m.groups]
    cw0 = [g.cache_weight.detach().clone() for g in m.groups]
    outs = m(idx, off)
    with torch.no_grad():
        refs = twin(idx, off)
    for k, (o, r) in enumerate(zip(outs, refs)):
        assert_close(o.detach().cpu().numpy(), r.cpu().numpy(), f"live output of table {k}")
    torch.stack(outs).sum().backward()
    torch.cuda.synchronize()
    assert all(not torch.equal(g.cache_weight.detach(), w) for g, w in zip(m.groups, cw0)), "both groups' cache rows moved"
    assert all(torch.equal(a.detach(), b) for a, b in zip(m.groups[1].tt_cores, cores0[1])), "all hits: the cores stay"
    assert all(not torch.equal(a.detach(), b) for a, b in zip(m.groups[0].tt_cores, cores0[0])), "misses train the cores"
    m.reset_cache()
    assert all(g.warmup and int((g.hashtbl >= 0).sum()) == 0 for g in m.groups)
