"""The shape-specialised backward's partial gradients as 16-byte stores (csrc/ttx_tt_spec.inc, Shape3::W16).

The exact r <= 32 kernels of a single sub-chunk compute d core_0 and the cooperative d core_1 TRANSPOSED -- the MFMA operands swapped, the same products
summed in the same order over K -- so that an accumulator's four registers are four consecutive floats of one partial row, and
store every partial as float4 in the flavour the launch chooses (write-through below kPartialWtBytes of partials, non-temporal
above).  ttx_debug_skip bit 18 (test library) runs the kernel as it was: products in the C/D layout, 4-byte non-temporal stores.

For every case, knob on against knob off: the dense gradients of all three cores, the SGD-updated and the Adagrad-updated cores
(and the Adagrad state) are BIT-IDENTICAL; knob off matches the oracle at util.assert_close's defaults; two runs of a case are
bit-identical.

Lookup counts 1, 15, 16, 17, 33, 64, 65, 200, all lookups of a table in ONE core-1 slice so that the count decides the chunks: a
chunk with three idle waves (1), a last group that is not a multiple of four (15), a full chunk (16), two chunks of one slice
(17 ..), and -- ttx_set_chunk(64), which in the test library asks for the sub-chunked kernel variant at any batch size -- the
sub-chunk walk with a partial last sub-chunk (65: 64 + 1; 200: three chunks of four sub-chunks and one of 8 lookups; the walk
keeps its 4-byte stores, profiles/partial_stores.md: here the knob must change nothing and the results must still be right).  The
lookups go into 8 bags per table, one of them empty, the others ragged."""
import numpy as np
import pytest
import torch

import gen_inputs as G
import oracle_lib as O
from util import LR, EPS, assert_adagrad_close, assert_close

pytestmark = pytest.mark.gpu

OLD_STORES = 1 << 18  # ttx_debug_skip: the 4-byte non-temporal stores
P = [5, 6, 7]
BAGS = 8
COUNTS = [1, 15, 16, 17, 33, 64, 65, 200]
GEOMS = {"q444r32": ([4, 4, 4], 32), "q444r16": ([4, 4, 4], 16), "q448r32": ([4, 4, 8], 32), "q244r32": ([2, 4, 4], 32)}


def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def make_case(q, rank, n, tables=1, seed=0):
    """n lookups per table, all in core-1 slice i1 = 2 + table (index = (i0 p1 + i1) p2 + i2), over 8 bags per table: bag 3
    empty, the others ragged"""
    rs = np.random.RandomState(1000 * seed + n)
    idx, lengths = [], []
    for k in range(tables):
        i0, i2 = rs.randint(0, P[0], n), rs.randint(0, P[2], n)
        idx.append((i0 * P[1] + (2 + k)) * P[2] + i2)
        cuts = np.sort(rs.randint(0, n + 1, BAGS - 2))
        ln = np.diff(np.concatenate([[0], cuts, [n]]))          # 7 ragged lengths (zeros allowed) that sum to n
        lengths.append(np.insert(ln, 3, 0))                     # ... and bag 3 empty
    idx = np.concatenate(idx).astype(np.int64)
    off = np.concatenate([[0], np.cumsum(np.concatenate(lengths))]).astype(np.int64)
    r = [1, rank, rank, 1]
    D = int(np.prod(q))
    return dict(tables=tables, p=P, q=q, r=r, B=BAGS, D=D, indices=idx, offsets=off,
                cores=G.make_cores(7 + n, tables, P, q, r, "signed"), d_out=G.make_grad(13 + n, tables, BAGS, D))


def run(c, mode, knob=0, chunk=0, psw=None, live=None):
    """one backward on the GPU -> the arrays the mode produces.  live: only the first `live` lookups count, told to the plan on
    the device (the padded-batch route); psw: per_sample_weights"""
    import tt_embeddings as E

    tables, p, q, r, B, D = c["tables"], c["p"], c["q"], c["r"], c["B"], c["D"]
    idx, off = t(c["indices"]), t(c["offsets"])
    Lt = torch.zeros(len(p), dtype=torch.int64, device=dev())
    e0, e1 = torch.empty(0, dtype=torch.int64, device=dev()), torch.empty(0, dtype=torch.int32, device=dev())
    if chunk:
        E.set_chunk(chunk)
    if knob:
        E.debug_skip(knob)
    try:
        colidx, rowidx, tableidx, ntt, _ = E.preprocess_indices_sync(idx, off, tables, True, e0, e1)
        nnz = idx.numel()
        n_dev = None if live is None else torch.tensor([live], dtype=torch.int32, device=dev())
        plan = E.make_plan(tables, p, q, r, nnz, colidx, tableidx, rowidx, n_dev=n_dev)
        cores = [t(x) for x in c["cores"]]
        d_out = t(c["d_out"])
        w = None if psw is None else t(psw)
        res = {}
        if mode == "dense":
            grads = E.tt_dense_backward(1000, D, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, cores, plan=plan, per_sample_weights=w)
            res["grads"] = [g.cpu().numpy() for g in grads]
        elif mode == "sgd":
            E.tt_sgd_backward(1000, D, LR, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, cores, plan=plan, per_sample_weights=w)
        else:
            state = [torch.zeros_like(x) for x in cores]
            E.tt_adagrad_backward(1000, D, LR, EPS, p, q, r, Lt, nnz, colidx, rowidx, tableidx, d_out, state, cores, plan=plan,
                                  per_sample_weights=w)
            res["state"] = [s.cpu().numpy() for s in state]
        res["cores"] = [x.cpu().numpy() for x in cores]
        return res
    finally:
        if knob:
            E.debug_skip(0)
        if chunk:
            E.set_chunk(0)


def oracle(c, mode, psw=None, live=None):
    """the CPU oracle on the same problem.  per_sample_weights: the oracle has none -- every lookup becomes a bag of its own whose
    gradient row is psw[n] * (its bag's row), the fp32 product the kernel forms on its way to LDS"""
    tables, B, D = c["tables"], c["B"], c["D"]
    g = O.make_geom(tables, c["p"], c["q"], c["r"])
    rowidx, tableidx = O.rowidx_from_offsets(c["offsets"], tables)
    idx, d_out = c["indices"], c["d_out"]
    if live is not None:
        idx, rowidx, tableidx = idx[:live], rowidx[:live], tableidx[:live]
    if psw is not None:
        assert tables == 1
        d_out = (np.asarray(psw, np.float32)[: idx.size, None] * c["d_out"][0][rowidx])[None]
        B, rowidx = idx.size, np.arange(idx.size, dtype=np.int64)
    cores = [x.copy() for x in c["cores"]]
    res = {}
    if mode == "dense":
        res["grads"] = O.tt_backward(g, O.OPTIM_DENSE, B, D, 0, 0, idx, rowidx, tableidx, d_out, cores)
    elif mode == "sgd":
        O.tt_backward(g, O.OPTIM_SGD, B, D, LR, 0, idx, rowidx, tableidx, d_out, cores)
    else:
        state = [np.zeros_like(x) for x in cores]
        O.tt_backward(g, O.OPTIM_ADAGRAD, B, D, LR, EPS, idx, rowidx, tableidx, d_out, cores, state)
        res["state"] = state
    res["cores"] = cores
    return res


def same(a, b, what):
    for key in a:
        for k, (x, y) in enumerate(zip(a[key], b[key])):
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), \
                f"{what}: {key}[{k}] differs in {int((x.view(np.uint32) != y.view(np.uint32)).sum())} of {x.size} values"


def check(c, what, chunk=0, psw=None, live=None):
    gref = oracle(c, "dense", psw, live)["grads"]
    for mode in ("dense", "sgd", "adagrad"):
        new = run(c, mode, 0, chunk, psw, live)
        again = run(c, mode, 0, chunk, psw, live)
        old = run(c, mode, OLD_STORES, chunk, psw, live)
        same(new, again, f"{what} {mode}: run to run")
        same(new, old, f"{what} {mode}: 16-byte stores against the 4-byte non-temporal ones")
        orc = oracle(c, mode, psw, live) if mode != "dense" else {"grads": gref}
        for k in range(3):
            if mode == "dense":
                assert_close(new["grads"][k], gref[k], f"{what} grad{k} vs oracle")
            elif mode == "sgd":
                assert_close(new["cores"][k], orc["cores"][k], f"{what} sgd core{k} vs oracle")
            else:
                assert_close(new["state"][k], orc["state"][k], f"{what} adagrad state{k} vs oracle")
                assert_adagrad_close(new["cores"][k], orc["cores"][k], gref[k], f"{what} adagrad core{k} vs oracle")


def test_the_knob_reaches_the_kernel_this_file_is_about():
    """the geometries run on the shape-specialised kernels (no generic tiles), and the test library carries the knob"""
    import tt_embeddings as E

    for name, (q, rank) in GEOMS.items():
        assert E.debug_tiles(1, P, q, [1, rank, rank, 1])["MC"] == 0, name
    E.debug_skip(OLD_STORES)
    try:
        assert E.hooks_lib().ttx_debug_state() & 1
    finally:
        E.debug_skip(0)
    assert E.hooks_lib().ttx_debug_state() == 0


@pytest.mark.parametrize("geom", list(GEOMS))
def test_single_sub_chunk_kernels(geom):
    q, rank = GEOMS[geom]
    for n in COUNTS:
        check(make_case(q, rank, n), f"{geom} n={n}")


@pytest.mark.parametrize("geom", list(GEOMS))
def test_sub_chunk_walk(geom):
    """ttx_set_chunk(64): plan chunks of four sub-chunks -- d core_1 carried across them in registers and stored once (4-byte
    non-temporal stores with the knob on or off)"""
    q, rank = GEOMS[geom]
    for n in (65, 200):
        check(make_case(q, rank, n), f"{geom} n={n} sub-chunks", chunk=64)


def test_per_sample_weights():
    c = make_case([4, 4, 4], 32, 33)
    psw = (np.random.RandomState(5).rand(33) * 2 - 0.5).astype(np.float32)
    check(c, "per_sample_weights n=33", psw=psw)
    check(c, "per_sample_weights n=33 sub-chunks", chunk=64, psw=psw)


def test_live_count_below_the_length():
    """the padded-batch route: the plan is told on the device that only the first 41 of 65 lookups count"""
    c = make_case([4, 4, 4], 32, 65)
    check(c, "41 of 65 live", live=41)
    check(c, "41 of 65 live, sub-chunks", chunk=64, live=41)


def test_three_tables():
    for q, rank in (([4, 4, 4], 32), ([2, 4, 4], 32)):
        check(make_case(q, rank, 33, tables=3), f"three tables q={q}")
