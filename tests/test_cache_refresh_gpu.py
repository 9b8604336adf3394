"""GPU tests of the cache refresh: ttx_cache_carry against the numpy restatement tests/carry_ref.py on tables
seated by the library's own insert with hand-written states, and `cache_populate(keep_trained=True, freq_shift=)` of the four
cached module kinds -- the arrays against carry_ref on a snapshot and a twin that takes the plain populate, the output of keys
cached before and after (bit-identical across the refresh; not so on the twin), and the ageing shift against a manual one.
Everything is a copy: every comparison is exact.

The kernel's tile is 256 slots and it walks at most 2048 tiles per pass; a row is moved by 2^k lanes in 16-byte units when
D % 4 == 0 and the arrays are 16-byte aligned, float by float otherwise: the sizes are the ones at which a bound, a group width or
a path changes."""
import copy

import numpy as np
import pytest
import torch

import carry_ref as CR
import oracle_lib as O
from test_pooling_modes_gpu import t
from util import EPS, LR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------------------------- the kernel
_TABLES = {}


def seated_table(H):
    """H // 3 keys where the library's own insert puts them, plus ONE key duplicated into the free slot behind it -> (hashtbl,
    the duplicate's slot, the slot of the findable copy); built once per size"""
    if H not in _TABLES:
        import tt_embeddings as E

        keys = np.unique(np.random.RandomState(H % 1000).randint(0, 1 << 40, size=H // 3, dtype=np.int64))
        ht = torch.full((H,), -1, dtype=torch.int64, device=DEV)
        E.update_cache_state(t(keys), ht, torch.zeros(H, dtype=torch.int64, device=DEV))
        tbl = ht.cpu().numpy()
        for s in np.nonzero(tbl != -1)[0]:
            home = O.hash64(int(tbl[s]), H)
            if tbl[(s + 1) % H] == -1 and (s - home) % H <= 1:  # (the next slot is free and inside the key's three probes)
                first, dup = int(s), int((s + 1) % H)
                break
        else:
            raise AssertionError("no key with a free slot behind it")
        tbl[dup] = tbl[first]
        assert O.hashtbl_find(int(tbl[first]), tbl) == first
        _TABLES[H] = (tbl, dup, first)
    return _TABLES[H]


def scene(H, cs, variant, seed):
    """-> (hashtbl, old_state, new_state, owners' rows).  `variant`: "mixed" (a two-row swap, kept and admitted owners), "all"
    (the swap, every owner kept) or "none" (every owner admitted)"""
    rs = np.random.RandomState(seed)
    tbl, dup, first = seated_table(H)
    occ = np.nonzero(tbl != -1)[0]
    occ = occ[occ != dup]
    empty = np.nonzero(tbl == -1)[0]
    nown = min(occ.size - 3, cs - 2)  # (two rows, at least, that no slot owns; three seated keys that own nothing)
    assert nown >= 5 and empty.size >= 3
    owners = rs.permutation(occ[occ != first])[:nown - 1].tolist() + [first]  # (the duplicated key owns a row too)
    newrows = rs.permutation(cs)[:nown]
    old, new = np.full(H, -1, np.int32), np.full(H, -1, np.int32)
    new[owners] = newrows
    outside = [-1, cs, -9, cs + 5, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    if variant == "none":
        old[owners] = [outside[i % len(outside)] for i in range(nown)]
    else:
        old[owners[0]], old[owners[1]] = newrows[1], newrows[0]  # the swap: m -> n, n -> m
        spare = [r for r in rs.permutation(cs) if r not in (newrows[0], newrows[1])]
        for i, s in enumerate(owners[2:]):
            old[s] = spare[i] if (variant == "all" or i % 2 == 0) else outside[i % len(outside)]
    rest = np.setdiff1d(occ, owners)  # seated keys whose new state names no row
    new[rest] = [outside[i % len(outside)] for i in range(rest.size)]
    old[rest] = rs.randint(0, cs, size=rest.size)
    new[empty], old[empty] = rs.randint(0, cs, size=empty.size), rs.randint(0, cs, size=empty.size)  # empty slots, states in range
    new[dup], old[dup] = newrows[2], newrows[3]  # the second copy of a key: its state collides with another slot's new row
    return tbl, old, new, newrows


def run_carry(tbl, old, new, ow, cw, oo, oq, offset=0):
    """-> (cache_weight, opt_state or None, inputs unchanged?) of E.cache_carry on device copies; offset: floats between a 16-byte
    boundary and the start of every float array"""
    import tt_embeddings as E

    def floats(a):
        if a is None:
            return None
        buf = torch.empty(a.size + offset, dtype=torch.float32, device=DEV)
        assert buf.data_ptr() % 16 == 0
        view = buf[offset:].view(a.shape)
        view.copy_(t(a))
        return view

    d = dict(tbl=t(tbl), old=t(old), new=t(new), ow=floats(ow), cw=floats(cw), oo=floats(oo), oq=floats(oq))
    E.cache_carry(d["tbl"], d["old"], d["new"], d["ow"], d["cw"], d["oo"], d["oq"])
    torch.cuda.synchronize()
    same = all(np.array_equal(d[k].cpu().numpy(), v) for k, v in (("tbl", tbl), ("old", old), ("new", new), ("ow", ow)))
    same = same and (oo is None or np.array_equal(d["oo"].cpu().numpy(), oo))
    return d["cw"].cpu().numpy(), None if oq is None else d["oq"].cpu().numpy(), same


def float_arrays(cs, D, sw, seed):
    rs = np.random.RandomState(seed)
    ow, cw = rs.rand(cs, D).astype(np.float32), rs.rand(cs, D).astype(np.float32) + 10
    shape = None if sw == 0 else ((cs,) if sw == 1 else (cs, D))
    oo = None if shape is None else rs.rand(*shape).astype(np.float32) + 20
    oq = None if shape is None else rs.rand(*shape).astype(np.float32) + 30
    return ow, cw, oo, oq


def check_case(H, cs, D, sw, offset=0):
    for v, variant in enumerate(("mixed", "all", "none")):
        tbl, old, new, newrows = scene(H, cs, variant, 7 * cs + v)
        ow, cw, oo, oq = float_arrays(cs, D, sw, D + v)
        want_w, want_s = CR.carry_ref(tbl, old, new, ow, cw, oo, oq)
        got_w, got_s, untouched = run_carry(tbl, old, new, ow, cw, oo, oq, offset)
        assert untouched, f"{variant}: the kernel wrote to one of its inputs"
        assert np.array_equal(got_w, want_w), variant
        assert sw == 0 or np.array_equal(got_s, want_s), variant
        # what the case holds, stated on the result: rows without an owner stay; the swap; kept / admitted as the variant says
        free = np.setdiff1d(np.arange(cs), newrows)
        assert free.size >= 2 and np.array_equal(got_w[free], cw[free]) and (sw == 0 or np.array_equal(got_s[free], oq[free]))
        part = CR.participants(tbl, old, new, cs)
        assert len(part) == newrows.size and sorted(p[1] for p in part) == sorted(newrows.tolist())
        kept = [p for p in part if p[2] >= 0]
        assert len(kept) == {"mixed": len(kept), "all": len(part), "none": 0}[variant]
        if variant == "mixed":
            assert 3 <= len(kept) < len(part)
        if variant != "none":
            a, b = int(newrows[0]), int(newrows[1])
            assert np.array_equal(got_w[a], ow[b]) and np.array_equal(got_w[b], ow[a]) and not np.array_equal(ow[a], ow[b])


@pytest.mark.parametrize("sw", ["none", "rowwise", "elementwise"])
@pytest.mark.parametrize("D", [4, 6, 16, 64, 260])
@pytest.mark.parametrize("cs", [7, 64, "H"])
@pytest.mark.parametrize("H", [257, 1000])
def test_carry_kernel_vs_reference(H, cs, D, sw):
    check_case(H, H if cs == "H" else cs, D, {"none": 0, "rowwise": 1, "elementwise": D}[sw])


@pytest.mark.parametrize("D,sw", [(16, 16), (64, 1), (4, 0)])
def test_carry_kernel_with_rows_off_the_16_byte_boundary(D, sw):
    """D % 4 == 0, but the arrays start 4 bytes behind a 16-byte boundary: float by float"""
    check_case(257, 64, D, sw, offset=1)


def test_carry_kernel_walks_more_tiles_than_it_has_work_groups():
    """2048 work-groups of 256 slots cover 2^19 slots in one pass: beyond that they come round again"""
    H = (1 << 19) + 700
    check_case(H, 1000, 8, 1)
    tbl, dup, first = seated_table(H)
    assert int(np.nonzero(tbl != -1)[0].max()) >= 1 << 19, "keys in the tiles of the second pass"


def test_carry_is_capturable_and_repeats_bit_for_bit():
    import tt_embeddings as E

    tbl, old, new, _ = scene(1000, 64, "mixed", 3)
    ow, cw, oo, oq = float_arrays(64, 64, 1, 5)
    want_w, want_s = CR.carry_ref(tbl, old, new, ow, cw, oo, oq)
    d = [t(a) for a in (tbl, old, new, ow, cw, oo, oq)]
    keep_w, keep_s = d[4].clone(), d[6].clone()
    E.cache_carry(*d)  # (warm: the code object is loaded outside the capture)
    torch.cuda.synchronize()
    d[4].copy_(keep_w), d[6].copy_(keep_s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.cache_carry(*d)
    for _ in range(2):
        d[4].copy_(keep_w), d[6].copy_(keep_s)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(d[4].cpu().numpy(), want_w) and np.array_equal(d[6].cpu().numpy(), want_s)


def test_shim_checks_its_tensors():
    import tt_embeddings as E

    tbl, old, new, _ = scene(257, 7, "mixed", 1)
    ow, cw, oo, oq = float_arrays(7, 6, 1, 2)
    ok = dict(hashtbl=t(tbl), old_state=t(old), cache_state=t(new), old_weight=t(ow), cache_weight=t(cw), old_opt_state=t(oo), opt_state=t(oq))
    bad = [dict(hashtbl=ok["hashtbl"].int()), dict(old_state=ok["old_state"].long()), dict(cache_state=ok["cache_state"][:-1]),
           dict(old_weight=ok["old_weight"].double()), dict(old_weight=ok["old_weight"][:, :4]), dict(cache_weight=ok["cache_weight"][:5]),
           dict(old_opt_state=None), dict(opt_state=None), dict(opt_state=ok["opt_state"][:5]), dict(old_opt_state=t(ow[:, :3])),
           dict(old_weight=ok["cache_weight"]), dict(old_opt_state=ok["opt_state"]),  # in place: refused by the library
           dict(hashtbl=ok["hashtbl"].cpu()), dict(old_weight=ok["old_weight"].cpu())]
    for change in bad:
        with pytest.raises(RuntimeError):
            E.cache_carry(**dict(ok, **change))
    torch.cuda.synchronize()
    assert np.array_equal(ok["cache_weight"].cpu().numpy(), cw) and np.array_equal(ok["opt_state"].cpu().numpy(), oq)


# --------------------------------------------------------------------------------------------------------------- the modules
P, Q, R = [20, 22, 25], [4, 4, 4], [16, 16]   # (tests/test_cache_gpu.py's three cores)
E_, D_ = 20 * 22 * 25, 64
P2, E2 = [10, 11, 12], 10 * 11 * 12          # the second cardinality of the mixed module
CS, HT = 30, 1024
KINDS = ["bag", "tables", "mixed", "unpooled"]
OPTIMS = ["sgd", "rowwise", "adagrad", "dense"]
NT = {"bag": 1, "tables": 3, "mixed": 2, "unpooled": 1}


def build(kind, optim):
    import tt_embeddings_ops as ops
    import ttx_mixed

    optimizer = {"sgd": ops.OptimType.SGD, "rowwise": ops.OptimType.EXACT_ROWWISE_ADAGRAD, "adagrad": ops.OptimType.EXACT_ADAGRAD,
                 "dense": ops.OptimType.SGD}[optim]
    kw = dict(optimizer=optimizer, sparse=optim != "dense", learning_rate=LR, eps=EPS, weight_dist="uniform", device=DEV,
              use_cache=True, cache_size=CS, hashtbl_size=HT)
    torch.manual_seed(4)
    if kind == "bag":
        return ops.TTEmbeddingBag(E_, D_, R, P, Q, **kw)
    if kind == "tables":
        return ops.TableBatchedTTEmbeddingBag(3, E_, D_, R, P, Q, **kw)
    if kind == "mixed":
        m = ttx_mixed.MixedTTEmbeddingBag([E_, E2], D_, R, [P, P2], Q, fused=True, **kw)
        assert len(m.groups) == 1 and m.groups[0].cache_weight.shape == (CS, D_)
        return m
    return ops.TTEmbedding(E_, D_, R, P, Q, **kw)


def inner(kind, m):
    """the module that owns the cache arrays"""
    return m.groups[0] if kind == "mixed" else m


def feed(kind, m, per_table):
    """one lookup per bag, table k looking up per_table[k] (tables with fewer lookups get empty bags behind them) -> the rows,
    table after table, [sum of the tables' lookups, D]"""
    B = max(len(i) for i in per_table)
    idx = [np.asarray(i, np.int64) for i in per_table]
    if kind == "unpooled":
        return m(t(idx[0]))
    starts = [np.minimum(np.arange(B + 1), i.size).astype(np.int64) for i in idx]
    if kind == "mixed":
        outs = m([t(i) for i in idx], [t(s[:-1]) for s in starts])
        return torch.cat([o[:i.size] for o, i in zip(outs, idx)])
    off = np.concatenate([[0]] + [s[1:] + sum(j.size for j in idx[:k]) for k, s in enumerate(starts)]).astype(np.int64)
    out = m(t(np.concatenate(idx)), t(off))
    out = out.reshape(len(idx), B, -1)
    return torch.cat([out[k, :i.size] for k, i in enumerate(idx)])


def key_of(kind, m, table, index):
    if kind == "tables":
        return table * m._key_stride() + index
    if kind == "mixed":
        return inner(kind, m)._key_space()[table] + index
    return index


def snapshot(c):
    state = c._cache_row_state()
    return dict(hashtbl=c.hashtbl.cpu().numpy(), freq=c.cache_freq.cpu().numpy(), state=c.cache_state.cpu().numpy(),
                weight=c.cache_weight.detach().cpu().numpy(), opt=None if state is None else state.cpu().numpy(),
                buffer=None if state is None else c.cache_optimizer_state.cpu().numpy())


_SCENARIOS = {}


def scenario(kind, optim):
    """count stream A (hot keys 0 .. 39 of every table), populate, three live training steps, count stream B (hot keys 20 .. 59);
    then the module takes cache_populate(keep_trained=True) and its twin the plain populate.  Built once per (kind, optimizer)."""
    if (kind, optim) in _SCENARIOS:
        return _SCENARIOS[(kind, optim)]
    nt = NT[kind]
    m = build(kind, optim)
    c = inner(kind, m)
    with torch.no_grad():
        feed(kind, m, [np.repeat(np.arange(40), 3)] * nt)
    m.cache_populate()
    assert not c.warmup and int((c.cache_state >= 0).sum()) == CS
    rs = np.random.RandomState(9)
    for _ in range(3):
        out = feed(kind, m, [np.arange(60)] * nt)
        out.backward(t(rs.rand(*out.shape).astype(np.float32) * 0.1))
        if optim == "dense":  # (no fused update: a plain SGD step on every parameter)
            with torch.no_grad():
                for par in m.parameters():
                    if par.grad is not None:
                        par -= LR * par.grad
                        par.grad = None
    with torch.no_grad():
        feed(kind, m, [np.repeat(np.arange(20, 60), 8)] * nt)
    torch.cuda.synchronize()
    snap = snapshot(c)
    before, twin = copy.deepcopy(m), copy.deepcopy(m)
    m.cache_populate(keep_trained=True)
    twin.cache_populate()
    torch.cuda.synchronize()
    after, plain = snapshot(c), snapshot(inner(kind, twin))
    part = CR.participants(after["hashtbl"], snap["state"], after["state"], CS)
    res = dict(m=m, twin=twin, before=before, snap=snap, after=after, plain=plain, part=part)
    _SCENARIOS[(kind, optim)] = res
    return res


@pytest.mark.parametrize("optim", OPTIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_refresh_keeps_trained_rows_and_their_state(kind, optim):
    s = scenario(kind, optim)
    snap, after, plain, part = s["snap"], s["after"], s["plain"], s["part"]
    # the inputs hold all three classes of keys
    kept, admitted = [p for p in part if p[2] >= 0], [p for p in part if p[2] < 0]
    evicted = [i for i in np.nonzero(snap["state"] >= 0)[0] if after["state"][i] < 0]
    assert len(kept) >= 5 and len(admitted) >= 5 and len(evicted) >= 5, (len(kept), len(admitted), len(evicted))
    assert len(part) == CS
    # the table is the plain populate's
    for name in ("hashtbl", "freq", "state"):
        assert np.array_equal(after[name], plain[name]), name
    # rows and state: the rule, applied to the snapshot and the plain populate's arrays
    assert (snap["opt"] is None) == (optim in ("sgd", "dense"))
    if snap["opt"] is not None:
        assert snap["opt"].shape == (CS,) and np.array_equal(plain["opt"], snap["opt"]), "a populate does not touch the state"
        assert (snap["opt"][[p[2] for p in kept]] > 0).all(), "precondition: the kept rows have a state"
    want_w, want_s = CR.carry_ref(after["hashtbl"], snap["state"], after["state"], snap["weight"], plain["weight"], snap["opt"], plain["opt"])
    assert np.array_equal(after["weight"], want_w)
    assert not np.array_equal(after["weight"], plain["weight"]), "precondition: the kept rows had moved away from the cores"
    if snap["opt"] is not None:
        assert np.array_equal(after["opt"], want_s)
        assert not after["opt"][[p[1] for p in admitted]].any() and (after["opt"][[p[1] for p in kept]] > 0).all()
        # (EXACT_ADAGRAD: the buffer is [cache_size, D], the rows' state its first cache_size floats; the rest is not touched)
        assert np.array_equal(after["buffer"].reshape(-1)[CS:], snap["buffer"].reshape(-1)[CS:])
    for _, n, mrow in kept:
        assert np.array_equal(after["weight"][n], snap["weight"][mrow])
    for _, n, _ in admitted:
        assert np.array_equal(after["weight"][n], plain["weight"][n])
    assert not inner(kind, s["m"]).warmup


@pytest.mark.parametrize("optim", OPTIMS)
@pytest.mark.parametrize("kind", KINDS)
def test_lookups_of_kept_keys_do_not_change_across_a_refresh(kind, optim):
    """a batch of keys cached before and after, one lookup per bag: bit-identical output before and after
    cache_populate(keep_trained=True); after the plain populate the rows are the cores' again"""
    s = scenario(kind, optim)
    m = s["m"]
    H = s["after"]["hashtbl"].size
    # (keys at their home slot: a cached key behind it can take a second seat when a live batch counts it, and is a miss from then on)
    keys = {int(s["after"]["hashtbl"][slot]) for slot, _, mrow in s["part"]
            if mrow >= 0 and O.hash64(int(s["after"]["hashtbl"][slot]), H) == slot}
    per_table = [[i for i in range(60) if key_of(kind, m, k, i) in keys] for k in range(NT[kind])]
    assert sum(len(i) for i in per_table) == len(keys) >= 5
    with torch.no_grad():
        out_before = feed(kind, s["before"], per_table)
        out_after = feed(kind, m, per_table)
        out_plain = feed(kind, s["twin"], per_table)
    torch.cuda.synchronize()
    assert out_before.shape == (len(keys), D_)
    assert torch.equal(out_before, out_after)
    assert not torch.equal(out_before, out_plain)
    assert (out_before != out_plain).any(dim=1).all(), "every kept row had been trained"


@pytest.mark.parametrize("kind", KINDS)
def test_freq_shift_equals_a_manual_shift(kind):
    s = scenario(kind, "sgd")
    m, twin = copy.deepcopy(s["before"]), copy.deepcopy(s["before"])
    c, ct = inner(kind, m), inner(kind, twin)
    assert int((c.cache_freq & 3).ne(0).sum()) > 0, "precondition: the shift drops set bits"
    m.cache_populate(freq_shift=2)
    ct.cache_freq >>= 2
    twin.cache_populate()
    torch.cuda.synchronize()
    a, b = snapshot(c), snapshot(ct)
    for name in ("hashtbl", "freq", "state", "weight"):
        assert np.array_equal(a[name], b[name]), name
    assert not np.array_equal(a["freq"], s["plain"]["freq"])
    # with keep_trained: the two keywords are independent
    m2, twin2 = copy.deepcopy(s["before"]), copy.deepcopy(s["before"])
    m2.cache_populate(keep_trained=True, freq_shift=2)
    inner(kind, twin2).cache_freq >>= 2
    twin2.cache_populate(keep_trained=True)
    torch.cuda.synchronize()
    a, b = snapshot(inner(kind, m2)), snapshot(inner(kind, twin2))
    for name in ("hashtbl", "freq", "state", "weight"):
        assert np.array_equal(a[name], b[name]), name


def test_refusal_and_warm_up_on_the_gpu():
    import tt_embeddings_ops as ops

    kw = dict(sparse=True, learning_rate=LR, weight_dist="uniform", device=DEV, use_cache=True, cache_size=CS, hashtbl_size=HT)
    torch.manual_seed(4)
    m = ops.TTEmbeddingBag(E_, D_, R, P, Q, reference_exact_populate=True, **kw)
    with pytest.raises(ValueError, match="reference_exact_populate"):
        m.cache_populate(keep_trained=True)
    assert m.warmup
    # still warming up: nothing to keep -- the plain populate
    m = ops.TTEmbeddingBag(E_, D_, R, P, Q, **kw)
    with torch.no_grad():
        feed("bag", m, [np.repeat(np.arange(40), 3)])
    twin = copy.deepcopy(m)
    m.cache_populate(keep_trained=True)
    twin.cache_populate()
    a, b = snapshot(m), snapshot(twin)
    for name in ("hashtbl", "freq", "state", "weight"):
        assert np.array_equal(a[name], b[name]), name
    assert not m.warmup
