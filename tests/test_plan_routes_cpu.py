"""tests/plan_ref.py, the host reference of the lookup plan, held on the CPU: against toy batches whose plan is written out by hand,
against the library's SOURCES (every constant of the route choice it mirrors), and -- the condition that keeps
tests/test_plan_routes_gpu.py honest -- its case table against plan_ref.route: every threshold has a case on each side, taking
the route the table names, and every route id is expected by at least one case."""
import os
import re

import numpy as np
import pytest

import plan_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbtt-embedding_amd", "csrc")


# ---- toy batches ------------------------------------------------------------------------------------------------------------------
def test_reference_on_a_hand_written_batch():
    """one table, p = [2, 3, 2] (L = [6, 2, 1]), five lookups with a duplicate: digits most significant first"""
    g = PR.Geom(1, [2, 3, 2])
    assert (g.S, g.idx32, g.mixed) == ([2, 3, 2], True, False)
    idx, tb, row = [7, 0, 11, 7, 4], [0] * 5, [0, 0, 1, 2, 2]
    e = PR.expected(g, idx, tb, row, mc=2)
    assert [x.tolist() for x in e["sid"]] == [[1, 0, 1, 1, 0], [0, 0, 2, 0, 2], [1, 0, 1, 1, 0]]
    assert [x.tolist() for x in e["perm"]] == [[1, 4, 0, 2, 3], [0, 1, 3, 2, 4], [1, 4, 0, 2, 3]]     # stable: equal keys in lookup order
    assert [x.tolist() for x in e["ipos"]] == [[2, 0, 3, 4, 1], [0, 1, 3, 2, 4], [2, 0, 3, 4, 1]]
    assert [x.tolist() for x in e["off"]] == [[0, 2, 5], [0, 3, 3, 5], [0, 2, 5]]
    assert e["lrec"].tolist() == [[0, 1, 1, 0], [1, 0, 0, 0], [3, 1, 1, 0], [2, 1, 1, 0], [4, 0, 0, 0]]
    assert e["lrow"].tolist() == [0, 0, 2, 1, 2]
    assert e["nchunks"] == 3 and e["hot"] == [0, 0, 0] and e["n"] == 5
    # a chunk list of it: slice 0 = positions [0, 3) in chunks of <= 2 (slots 0, 1), slice 2 = [3, 5) (slot 2); any dispatch order
    rec = np.array([[2, 3, 2, 2], [0, 0, 2, 0], [0, 2, 1, 1], [0, 0, 0, 0]])
    PR.check_chunks(e, 2, 3, rec, [0, 2, 2, 3])
    for bad, why in (([[2, 3, 2, 2], [0, 0, 2, 0], [0, 1, 1, 1]], "overlap"), ([[2, 3, 2, 2], [0, 0, 1, 0], [0, 2, 1, 1]], "gap"),
                     ([[2, 3, 2, 2], [0, 0, 2, 0], [0, 2, 1, 0]], "slot twice"), ([[2, 3, 2, 2], [0, 0, 3, 0], [0, 3, 0, 1]], "count"),
                     ([[2, 3, 1, 2], [0, 0, 2, 0], [0, 2, 1, 1]], "short slice"), ([[1, 3, 2, 2], [0, 0, 2, 0], [0, 2, 1, 1]], "wrong slice")):
        with pytest.raises(AssertionError):
            PR.check_chunks(e, 2, 3, np.array(bad), [0, 2, 2, 3])
            pytest.fail(f"check_chunks accepted a list with a {why}")
    with pytest.raises(AssertionError):
        PR.check_chunks(e, 2, 3, rec, [0, 2, 3, 3])


def test_reference_clamps_as_the_library_and_adds_the_table():
    """two tables of p = [2, 3, 2]: a negative index is index 0, an index beyond the table is clamped in core 0 only (the other cores
    take idx / L % p of the index as it is), and table k's slices lie behind those of the tables in front of it"""
    g = PR.Geom(2, [2, 3, 2])
    assert g.S == [4, 6, 4]
    sid = PR.slice_ids(g, [-5, 12, 5], [1, 0, 1])
    assert [x.tolist() for x in sid] == [[2, 1, 2], [3, 0, 5], [2, 0, 3]]
    e = PR.expected(g, [-5, 12, 5], [1, 0, 1], [4, 5, 6], mc=16)
    assert e["off"][1].tolist() == [0, 1, 1, 1, 2, 2, 3] and e["lrec"].tolist() == [[1, 1, 0, 0], [0, 2, 2, 0], [2, 2, 3, 0]]
    assert e["lrow"].tolist() == [5, 4, 6]


def test_reference_decodes_mixed_tables_with_their_own_factors():
    g = PR.Geom(2, [[2, 3], [3, 2]])
    assert g.mixed and not g.idx32 and g.S == [5, 5] and g.p_max == [3, 3] and [b.tolist() for b in g.base] == [[0, 2], [0, 3]]
    sid = PR.slice_ids(g, [5, 5, 0], [1, 0, 1])
    assert [x.tolist() for x in sid] == [[4, 1, 2], [4, 2, 3]]


def test_hot_counts_and_chunk_totals():
    """the thresholds of hdr[8 + t]: a thin slice is hot at MORE than 512 lookups, a pivot slice at more than 16 chunks"""
    g = PR.Geom(1, [3, 3])                                     # idx = 3 i0 + i1
    idx = np.concatenate([np.full(513, 0), np.full(512, 3), np.full(16 * 4 + 1, 7), np.full(16 * 4, 8)])   # slices 0, 1, 2 of core 0
    e = PR.expected(g, idx, np.zeros(idx.size, dtype=np.int64), np.zeros(idx.size, dtype=np.int64), mc=4)
    assert e["lens"][0].tolist() == [513, 512, 129] and e["hot"][0] == 1
    assert e["lens"][1].tolist() == [1025, 65, 64] and e["hot"][1] == 2 and e["nchunks"] == 257 + 17 + 16


def test_route_on_hand_written_shapes():
    one, two = PR.Geom(1, [7, 6, 5]), PR.Geom(40, [200, 6, 5])
    assert PR.route(one, 1, 16) == PR.TINY and PR.route(one, 1, 16, n_dev=True) == PR.SINGLE
    assert PR.route(one, 5000, 16, entry="prologue", nb=10) == PR.SINGLE_PROLOGUE and PR.route(one, 5000, 16, entry="prologue", nb=5000) == PR.SINGLE
    assert PR.route(one, 20000, 16, entry="prologue", nb=10) == PR.UNITS and PR.route(one, 5000, 16, entry="multi", nb=10) == PR.MULTIBATCH
    assert PR.route(two, 5000, 16) == PR.MULTIPASS + 2 and PR.route(two, 5000, 16, entry="prologue", nb=400) == PR.GROUPED10
    assert PR.group_shape(two, 5000) == (2, 20, 400, 1)
    assert PR.route(PR.Geom(1, [3000, 6, 5]), 300000, 1) == PR.MULTIPASS + 2        # (MC = 1: 300,000 full chunks do not fit finish_wide's count)
    assert PR.route(PR.Geom(1, [3000, 6, 5]), 300000, 16) == PR.WIDE12
    assert [PR.passes_of(s) for s in (1, 2, 256, 257, 65536, 65537, 1 << 24, (1 << 24) + 1)] == [1, 1, 1, 2, 2, 3, 3, 4]
    assert [PR.unit_positions(n) for n in (16385, 65536, 65537, 1 << 20)] == [256, 256, 320, 4096]
    assert sorted(set(PR.route_family(r) for r in PR.ALL_ROUTES)) == ["multi-pass", "single", "table groups", "tiny", "units", "wide"]


# ---- the constants, pinned to the sources ---------------------------------------------------------------------------------------
def _squeeze(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return re.sub(r"\s+", "", text)


def _constexpr(text, name):
    m = re.search(r"constexpr\s+int\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, f"constexpr int {name} not found"
    return m.group(1).strip()


def test_route_constants_match_the_sources():
    """plan_ref.route restates plan_build / plan_build_mb / prologue_fusable: a retune of one of their constants,
    or a change in the order of their choices, must fail HERE -- otherwise the cases of tests/test_plan_routes_gpu.py would
    quietly stop standing on both sides of a threshold"""
    plan = open(os.path.join(CSRC, "ttx_plan.hip")).read()
    internal = open(os.path.join(CSRC, "ttx_internal.h")).read()
    hooks = open(os.path.join(ROOT, "include", "ttx_test_hooks.h")).read()
    sq = _squeeze(plan)
    assert int(_constexpr(internal, "kWave")) == PR.WAVE
    assert int(_constexpr(plan, "kOneMaxN")) == PR.ONE_MAX_N and int(_constexpr(plan, "kProMaxBags")) == PR.PRO_MAX_BAGS
    assert _constexpr(plan, "kWideSpan") == "kWideThreads * kSB" and int(_constexpr(plan, "kWideThreads")) * int(_constexpr(plan, "kSB")) == PR.WIDE_SPAN
    assert int(_constexpr(plan, "kWideMaxG")) == PR.WIDE_MAX_G and int(_constexpr(plan, "kMbFuseU")) == PR.MB_FUSE_U
    assert _constexpr(plan, "kMaxGroups") == "kMaxGroupsHost" and int(_constexpr(plan, "kMaxGroupsHost")) == PR.MAX_GROUPS
    assert int(_constexpr(internal, "kMaxMulti")) == PR.MAX_MULTI
    assert int(re.search(r"#define\s+TTX_SEG_THIN\s+(\d+)", internal).group(1)) == PR.SEG_THIN
    assert int(re.search(r"#define\s+TTX_HOT_PIVOT\s+(\d+)", internal).group(1)) == PR.HOT_PIVOT
    # plan_build: the tiny limit and what else leaves the tiny route
    assert f"if(nnz>{PR.TINY_MAX_N}||!d.idx32||n_dev)returnplan_build_mb(" in sq
    # plan_build_mb, in its order: single launch; one wide digit; table groups; 8-bit passes; wave units
    marks = [
        "if(maxp==1&&N<=kOneMaxN&&!d.tab){",
        f"if((maxp>1||d.tab)&&(N+kWideSpan-1)/kWideSpan<=kWideMaxG&&N/(P.MC>0?P.MC:1)<(1<<{PR.FULL_CHUNK_LIMIT.bit_length() - 1})){{",
        *[f"if(smax<={span})returnplan_build_wide<{bits},false>(" for bits, span in PR.WIDE_DIGITS],
        "if(offsets&&d.num_tables>1&&maxp>1){",
        "intgsz=(d.num_tables+kMaxGroups-1)/kMaxGroups;constintngroups=(d.num_tables+gsz-1)/gsz;constlonglongrows_per_group=(longlong)N/kWideSpan/ngroups+1;",
        f"if((longlong)gsz*pmax<={PR.GROUP_DIGITS[1][1]}&&rows_per_group<=kWideMaxG){{",
        f"(longlong)gsz*pmax<={PR.GROUP_DIGITS[0][1]}?plan_build_wide<{PR.GROUP_DIGITS[0][0]},true>(",
        f":plan_build_wide<{PR.GROUP_DIGITS[1][0]},true>(",
        f"if(maxp>1||N>kMbFuseU*{PR.UNIT_MAX}||d.tab){{",
        "A.unit=256;if((N+255)/256>kMbFuseU)A.unit=((N+kMbFuseU-1)/kMbFuseU+63)/64*64;",
    ]
    at = sq.index("staticintplan_build_mb(")
    for mk in marks:
        nxt = sq.find(mk, at)
        assert nxt >= 0, f"plan_build_mb no longer reads `{mk}` (in this order): update tests/plan_ref.py::route"
        at = nxt
    assert "passes[t]=(bits+7)/8>0?(bits+7)/8:1;" in sq and "while((1ll<<bits)<d.S[t])++bits;" in sq
    # prologue_fusable, plan_batches_ok
    assert ("if(d.num_tables!=1||!(nnz>1024&&nnz<=kOneMaxN)||nb<1||nb>kProMaxBags)returnfalse;for(intt=0;t<d.T;++t)if(d.S[t]>256)returnfalse;"
            "returntrue;") in sq
    assert PR.TINY_MAX_N == 1024 and PR.ONE_DIGIT == 256
    # the 32-bit decode: prod(p) <= 2^32, never for tables of different row factors (make_dims)
    api = _squeeze(open(os.path.join(CSRC, "ttx_api.hip")).read())
    assert "d->idx32=Lv<=(1ll<<32);" in api and "Lv=1ll<<40;" in api
    # the route ids
    ids = {k: int(v) for k, v in re.findall(r"#define\s+TTX_ROUTE_([A-Z_]+)\s+(\d+)", hooks)}
    assert ids == dict(TINY=PR.TINY, SINGLE=PR.SINGLE, SINGLE_PROLOGUE=PR.SINGLE_PROLOGUE, UNITS=PR.UNITS, WIDE=PR.WIDE, GROUPED=PR.GROUPED,
                       MULTIPASS=PR.MULTIPASS, MULTIBATCH=PR.MULTIBATCH)
    assert "TTX_PLAN_ROUTE((GRP?TTX_ROUTE_GROUPED:TTX_ROUTE_WIDE)+BITS);" in sq and "TTX_PLAN_ROUTE(TTX_ROUTE_MULTIPASS+maxp);" in sq


def test_the_tiny_route_holds_one_batch_per_wave():
    """plan_build's tiny branch launches ONE instantiation of plan_small_kernel: with 16 waves and at most 1024 lookups a wave holds
    at most one batch of 64 (nb <= 1), whatever the count -- the arithmetic of the launch, for every count the route takes"""
    plan = open(os.path.join(CSRC, "ttx_plan.hip")).read()
    waves = int(_constexpr(plan, "kPlanThreads")) // PR.WAVE
    for n in range(0, PR.TINY_MAX_N + 1):
        per = ((n + waves - 1) // waves + PR.WAVE - 1) // PR.WAVE * PR.WAVE
        assert per // PR.WAVE <= 1
    assert sorted(set(re.findall(r"plan_small_kernel<(\d+)>", plan))) == ["2"]
    # (the duplicate map's one-work-group sort takes up to kDedupMaxN lookups: all of ITS instantiations are reached)
    dmax = int(_constexpr(open(os.path.join(CSRC, "ttx_internal.h")).read(), "kDedupMaxN"))
    nbs = {(((n + waves - 1) // waves + PR.WAVE - 1) // PR.WAVE) for n in (1, 2049, 4097, 8193, 12289, dmax)}
    assert nbs == {1, 3, 5, 9, 13, 16}


# ---- the case table of the GPU file ------------------------------------------------------------------------------------------------
def test_case_table_stands_on_both_sides_of_every_threshold():
    import test_plan_routes_gpu as GPU

    names = [c["name"] for c in GPU.CASES]
    assert len(set(names)) == len(names)
    derived = [GPU.Derived(c) for c in GPU.CASES]
    for label, near, near_routes, far, far_routes in GPU.THRESHOLDS:
        for side, pred, routes in (("near", near, near_routes), ("far", far, far_routes)):
            hit = [d for d in derived if pred(d)]
            assert hit, f"{label}: no case on the {side} side"
            for d in hit:
                assert d.route in routes, (f"{label}: case {d.name} ({side} side) takes route {PR.route_name(d.route)}, "
                                           f"the table expects {sorted(PR.route_name(r) for r in routes)}")
    # the near ("at capacity") side of every threshold carries EVERY stream -- "every slice used" only where there are at least as
    # many lookups as slice ids
    for label, near, _, far, _ in GPU.THRESHOLDS:
        for d in derived:
            if near(d):
                need = set(GPU.FULL) - ({"each_once"} if d.smax > d.N else set())
                assert need <= set(d.c["streams"]), f"{label}: case {d.name} lacks the streams {sorted(need - set(d.c['streams']))}"
    # sizes that are no multiple of 64 meet a skewed stream on the one-pass routes as well
    for name in ("single-16385", "units-65537", "units-1048577"):
        d = next(x for x in derived if x.name == name)
        assert d.N % 64 and set(GPU.FAR_SKEWED) <= set(d.c["streams"])
    # no bag rows: once per place that writes hdr[3]
    assert {d.route for d in derived if not d.c["rows"]} == {PR.TINY, PR.SINGLE, PR.UNITS, PR.WIDE10, PR.MULTIPASS + 2}
    seen = {d.route for d in derived}
    assert seen == set(PR.ALL_ROUTES), f"routes no case expects: {sorted(PR.route_name(r) for r in set(PR.ALL_ROUTES) - seen)}"
    # a device-side count of 0, 1, N - 1, N behind four thresholds
    for tag in ("single", "units", "wide", "passes"):
        lives = sorted(d.live for d in derived if d.name.startswith(f"dev-{tag}-"))
        n = next(d.N for d in derived if d.name.startswith(f"dev-{tag}-"))
        assert lives == [0, 1, n - 1, n]
    # every stream the GPU file knows is used, and nothing above the end-to-end limit is small by accident
    streams = {s for c in GPU.CASES for s in c["streams"]}
    assert streams == set(GPU.FULL) | {"clamp"}
    assert max(c["N"] for c in GPU.CASES) == (1 << 20) + 1


def test_streams_are_what_their_names_say():
    import test_plan_routes_gpu as GPU

    c = next(x for x in GPU.CASES if x["name"] == "S-256")
    g = PR.Geom(c["tables"], c["p"])
    mc = GPU.MC_NOMINAL
    for stream in GPU.FULL:
        idx, off = GPU.make_batch(c, stream, mc)
        assert idx.size == c["N"] and off.size == c["tables"] * c["B"] + 1 and off[0] == 0 and off[-1] == c["N"] and (np.diff(off) >= 0).all()
        assert (np.diff(off) == 0).any(), "some bags are empty"
        assert (idx >= 0).all() and (idx < g.rows[0]).all()
        lens = PR.expected(g, idx, np.zeros(idx.size, dtype=np.int64), np.zeros(idx.size, dtype=np.int64), mc)["lens"]
        if stream == "one_slice":
            assert all((ln > 0).sum() == 1 for ln in lens)
        if stream == "each_once":
            assert all((ln > 0).all() and ln.max() - ln.min() <= 1 for ln in lens)
        if stream == "ends_empty":
            assert all(ln[0] == 0 and ln[-1] == 0 and ln.sum() == c["N"] for ln in lens)
        if stream == "ends_only":
            assert all(ln[0] > 0 and ln[-1] > 0 and ln[0] + ln[-1] == c["N"] for ln in lens)
        if stream == "pivot_runs":
            assert lens[1][:4].tolist() == [mc, mc + 1, 3 * mc, 17 * mc + 1]
    idx, _ = GPU.make_batch(c, "clamp", mc)
    assert (idx < 0).sum() == 2 and (idx >= g.rows[0]).sum() == 2
    assert np.array_equal(GPU.make_batch(c, "uniform", mc)[0], GPU.make_batch(c, "uniform", mc)[0])
