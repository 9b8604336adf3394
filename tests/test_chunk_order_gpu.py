"""The pivot's DISPATCH order on the one-launch and the wide plan routes (csrc/ttx_plan.hip: finish_single_pass, finish_wide).

The index of a chunk's record in chunk_rec is the blockIdx of its contraction work-group, and work-groups go round-robin over
the 8 XCDs, each with an L2 of its own.  The two routes deal the chunk slots (slice-major) column-major over 8 columns
(tests/chunk_order_ref.py), so that the chunks of one core_1 slice share `index % 8` -- one XCD fetches the slice once --
unless the slice straddles one of the 7 segment boundaries.  The order is performance only: ttx_debug_skip bit 17 (test
library) builds the same plan with ONE column, the list in slot order, and every result must be bit-identical.

Every case is built through the test library as tests/test_plan_routes_gpu.py does (its helpers are used here), once with 8
columns and once with one.  Checked per case:
  1. plan_ref.check_chunks (inside check_plan): the list is a permutation of the slots that tiles every slice;
  2. the counts of index % 8 over [0, hdr[0]) differ by at most 1;
  3. distinct (index % 8, slice) pairs <= non-empty slices + 7;
  4. for every pair the rows index // 8 of its chunks are consecutive;
  5. the index of every slot equals the CPU mirror's (chunk_order_ref.dispatch_index on plan_ref.expected), for which 2 and 3
     are checked on the CPU too; where PARENT_VIOLATES says so, the order before the columns (all full chunks slice-major,
     then the partial ones: chunk_order_ref.full_first_index) has MORE pairs than the bound;
  6. with one column index == slot for every chunk;
  7. at the benchmark's geometry: forward output, dense gradients and the cores after one fused SGD step bit-identical
     between the two plans.
N = 5 is built twice: through ttx_plan_build it takes the tiny route (plan_small_kernel, not changed: slot order, which is also
what fewer than 8 chunks give), and through ttx_plan_build_n with buffers for 1025 lookups it takes the single launch with 5
live lookups -- fewer than 8 chunks on the route under test."""
import ctypes as C

import numpy as np
import pytest
import torch

import chunk_order_ref as CO
import gen_inputs as G
import plan_ref as PR
import test_plan_routes_gpu as TP

pytestmark = pytest.mark.gpu

P3, WIDE_P = TP.P3, [300, 6, 5]
BENCH = dict(p=[200, 220, 250], q=[4, 4, 4], r=[1, 32, 32, 1], B=128, L=20)

CASES = [TP.case(f"order-single-{n}", 1, P3, n, ("uniform", "one_slice", "pivot_runs", "ends_only")) for n in (3000, 16384)]
CASES += [
    TP.case("order-tiny-5", 1, P3, 5, ("uniform",)),
    TP.case("order-single-live-5", 1, P3, 1025, ("uniform",), entry="build_n", live=5),
    TP.case("order-wide-3000", 1, WIDE_P, 3000, ("uniform", "ends_only")),
]
ROUTES = {"order-single-3000": PR.SINGLE, "order-single-16384": PR.SINGLE, "order-tiny-5": PR.TINY, "order-single-live-5": PR.SINGLE,
          "order-wide-3000": PR.WIDE10}
# cases whose stream gives some slice several chunks at consecutive list indices of the earlier order
PARENT_VIOLATES = {("order-single-3000", "uniform"), ("order-single-16384", "uniform"), ("order-single-3000", "pivot_runs"),
                   ("order-single-16384", "pivot_runs"), ("order-single-3000", "ends_only"), ("order-single-16384", "ends_only"),
                   ("order-wide-3000", "uniform"), ("order-wide-3000", "ends_only")}
PARAMS = [(c, s) for c in CASES for s in c["streams"]]


def build(E, c, ti, toff, trow, ttab, mask):
    """one plan through the test library with ttx_debug_skip(mask) -> (buffer, route id)"""
    E.debug_skip(mask)
    try:
        assert (E.hooks_lib().ttx_debug_state() & 1) == (1 if mask else 0), "ttx_debug_state() does not report the knob"
        buf, route, _, _ = TP.build_plan(E, c, ti, toff, trow, ttab, 0xA5)
    finally:
        E.debug_skip(0)
    return buf, route


def chunk_list(lay, buf):
    v = buf.view(torch.int32)
    hdr0 = int(v[lay["hdr"][0]])
    o, ln = lay["chunk_rec"]
    return v[o:o + ln].cpu().numpy().reshape(-1, 4)[:hdr0].astype(np.int64)


def check_columns(rec, exp, mc, what, parent_violates=False):
    """2 - 5 of the module docstring for the 8-column list `rec` = {slice, start, count, slot} in list order"""
    n = rec.shape[0]
    lens1 = exp["lens"][1]
    nonempty = int((lens1 > 0).sum())
    # 5. the CPU side: the mirror's order of the expected slots, and its bounds
    sl = CO.slot_slices(lens1, mc)
    assert sl.size == n == exp["nchunks"]
    want = CO.dispatch_index(np.arange(n), n)
    cnt = np.bincount(want % CO.COLS, minlength=CO.COLS)
    cpu_pairs = len(CO.pairs(want, sl))
    before = len(CO.pairs(CO.full_first_index(lens1, mc), sl))
    print(f"[chunk-order] {what}: {n} chunks of {nonempty} slices; (index % 8, slice) pairs {cpu_pairs} (bound {nonempty + CO.COLS - 1}), "
          f"full-chunks-first order {before}")
    assert n == 0 or cnt.max() - cnt.min() <= 1
    assert cpu_pairs <= nonempty + CO.COLS - 1
    if parent_violates:
        assert before > nonempty + CO.COLS - 1, f"{what}: the earlier order already meets the bound: the case shows nothing"
    if n == 0:
        return
    index, s, slot = np.arange(n), rec[:, 0], rec[:, 3]
    got = np.empty(n, dtype=np.int64)
    got[slot] = index   # (check_chunks: the slots are a permutation)
    assert np.array_equal(got, want), f"{what}: the list is not the slots dealt column-major over 8 columns"
    # 2.
    cnt = np.bincount(index % CO.COLS, minlength=CO.COLS)
    assert cnt.max() - cnt.min() <= 1, f"{what}: chunks per residue {cnt.tolist()}"
    # 3.
    pr = CO.pairs(index, s)
    assert len(pr) <= nonempty + CO.COLS - 1, f"{what}: {len(pr)} (index % 8, slice) pairs for {nonempty} non-empty slices"
    # 4.
    for r, sv in pr:
        rows = np.sort(index[(index % CO.COLS == r) & (s == sv)] // CO.COLS)
        assert np.array_equal(rows, rows[0] + np.arange(rows.size)), f"{what}: slice {sv} in column {r} has rows {rows.tolist()}"


def check_slot_order(rec, what):
    assert np.array_equal(rec[:, 3], np.arange(rec.shape[0])), f"{what}: one column, but the list is not in slot order"


@pytest.mark.parametrize("c,stream", PARAMS, ids=[f"{c['name']}-{s}" for c, s in PARAMS])
def test_chunks_of_a_slice_share_a_column(c, stream):
    import tt_embeddings as E

    what = f"{c['name']}/{stream}"
    g = PR.Geom(c["tables"], c["p"])
    N = c["N"]
    lay = E.debug_plan_layout(c["tables"], c["p"], c["q"], c["r"], N)
    mc = lay["MC"]
    assert mc == TP.MC_NOMINAL
    idx, off = TP.make_batch(c, stream, mc)
    rowidx, tableidx, exp = TP.reference(c, g, idx, off, mc)
    ti, toff, trow, ttab = TP.t(idx), TP.t(off), TP.t(rowidx), TP.t(tableidx)
    for mask, cols in ((0, 8), (CO.ONE_COLUMN, 1)):
        buf, route = build(E, c, ti, toff, trow, ttab, mask)
        assert route == ROUTES[c["name"]], f"{what}: route {PR.route_name(route)}"
        TP.check_plan(lay, buf, exp, route, g, mc, f"{what} ({cols} columns)")
        rec = chunk_list(lay, buf)
        if cols == 8 and route != PR.TINY:
            check_columns(rec, exp, mc, what, parent_violates=(c["name"], stream) in PARENT_VIOLATES)
        else:
            check_slot_order(rec, what)
        if c["name"].endswith("-5"):
            assert rec.shape[0] < CO.COLS
            check_slot_order(rec, what)   # fewer than 8 chunks: the identity with 8 columns too
    assert E.lib().ttx_debug_state() == 0


def test_multi_batch_launch_orders_every_shifted_plan():
    """ttx_lookup_prologue_multi, 16 batches of 2000 in one launch: finish_single_pass writes batch z's list z plan strides behind
    batch 0's"""
    import tt_embeddings as E

    c = TP.case("order-multi-16", 1, P3, 2000, TP.FULL, entry="multi", B=64, nbatch=16)
    g = PR.Geom(c["tables"], c["p"])
    N, nbatch, d = c["N"], c["nbatch"], TP.dev()
    lay = E.debug_plan_layout(c["tables"], c["p"], c["q"], c["r"], N)
    mc = lay["MC"]
    one = dict(c, entry="prologue")
    batches = [TP.make_batch(c, c["streams"][z % len(c["streams"])], mc, salt=z) for z in range(nbatch)]
    tis, toffs = [TP.t(b[0]) for b in batches], [TP.t(b[1]) for b in batches]
    refs = [TP.reference(one, g, idx, off, mc)[2] for idx, off in batches]
    gg = E._geom(c["tables"], c["p"], c["q"], c["r"])
    for mask, cols in ((0, 8), (CO.ONE_COLUMN, 1)):
        E.debug_skip(mask)
        try:
            with E.test_library() as L:
                L.ttx_lookup_prologue_multi.argtypes = [C.POINTER(type(gg)), C.c_int32, C.c_int64, C.POINTER(C.c_void_p), C.c_int64,
                                                        C.POINTER(C.c_void_p), C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_size_t, C.c_void_p]
                stride = (L.ttx_plan_bytes(C.byref(gg), N) + 255) // 256 * 256
                plans = torch.full((nbatch * stride,), 0x5A, dtype=torch.uint8, device=d)
                rows = torch.full((nbatch * N,), -7, dtype=torch.int64, device=d)
                tabs = torch.full((nbatch * N,), -7, dtype=torch.int64, device=d)
                E._check(L.ttx_lookup_prologue_multi(C.byref(gg), nbatch, N, E._ptr_array(tis), c["tables"] * c["B"], E._ptr_array(toffs), 0,
                                                     None, None, TP._vp(rows), TP._vp(tabs), TP._vp(plans), stride,
                                                     C.c_void_p(E._stream(d))))
                route = E.debug_plan_route()
        finally:
            E.debug_skip(0)
        torch.cuda.synchronize()
        assert route == PR.MULTIBATCH
        for z in range(nbatch):
            what = f"{c['name']} batch {z} ({cols} columns)"
            pz = plans[z * stride:(z + 1) * stride]
            TP.check_plan(lay, pz, refs[z], route, g, mc, what)
            rec = chunk_list(lay, pz)
            if cols == 8:
                check_columns(rec, refs[z], mc, what)
            else:
                check_slot_order(rec, what)


def test_benchmark_geometry_results_do_not_depend_on_the_order():
    """p = [200, 220, 250], q = [4, 4, 4], ranks 32, 2560 lookups in 128 bags: the plan's order, and forward output, dense gradients
    and the cores after one fused SGD step bit for bit between 8 columns and one"""
    import tt_embeddings as E

    p, q, r, B, Lb = BENCH["p"], BENCH["q"], BENCH["r"], BENCH["B"], BENCH["L"]
    N, D, E_rows = B * Lb, int(np.prod(q)), int(np.prod(p))
    c = TP.case("order-bench-2560", 1, p, N, ("uniform",), B=B, q=q, r=r)
    g = PR.Geom(1, p)
    lay = E.debug_plan_layout(1, p, q, r, N)
    mc = lay["MC"]
    idx, off = G.make_requests(1235, 1, B, 1, Lb, E_rows)[0]
    rowidx, tableidx, exp = TP.reference(c, g, idx, off, mc)
    ti, toff, trow, ttab = TP.t(idx), TP.t(off), TP.t(rowidx), TP.t(tableidx)
    cores = G.make_cores(31, 1, p, q, r[1:-1])
    d_out = TP.t(G.make_grad(33, 1, B, D))
    Lt = torch.zeros(3, dtype=torch.int64, device=TP.dev())
    res = []
    for mask, cols in ((0, 8), (CO.ONE_COLUMN, 1)):
        buf, route = build(E, c, ti, toff, trow, ttab, mask)
        assert route == PR.SINGLE
        TP.check_plan(lay, buf, exp, route, g, mc, f"{c['name']} ({cols} columns)")
        rec = chunk_list(lay, buf)
        if cols == 8:
            check_columns(rec, exp, mc, c["name"], parent_violates=True)
        else:
            check_slot_order(rec, c["name"])
        assert E.lib().ttx_debug_state() == 0   # both plans run on the same library at its own settings
        plan = E.Plan(buf, N, None)
        dc = [TP.t(x) for x in cores]
        out = E.tt_forward(1000, 1, B, D, p, q, r, Lt, N, ti, trow, ttab, dc, plan=plan)
        grads = E.tt_dense_backward(1000, D, p, q, r, Lt, N, ti, trow, ttab, d_out, dc, plan=plan)
        E.tt_sgd_backward(1000, D, 0.1, p, q, r, Lt, N, ti, trow, ttab, d_out, dc, plan=plan)
        torch.cuda.synchronize()
        res.append((out.cpu(), [x.cpu() for x in grads], [x.cpu() for x in dc]))
    (o8, g8, c8), (o1, g1, c1) = res
    assert o8.abs().max() > 0 and all(x.abs().max() > 0 for x in g8)
    assert torch.equal(o8, o1), "forward output differs between 8 columns and one"
    for k in range(3):
        assert torch.equal(g8[k], g1[k]), f"dense gradient of core {k} differs between 8 columns and one"
        assert torch.equal(c8[k], c1[k]), f"core {k} after a fused SGD step differs between 8 columns and one"
        assert not torch.equal(c8[k], torch.from_numpy(cores[k])), f"core {k}: the SGD step changed nothing"
