"""Cases of tests/test_entry_chain_gpu.py: the single-sub-chunk contraction kernels at the smallest shape of the specialised
family, with chunk lengths forced through the pivot slices.  TEST INFRASTRUCTURE.

Geometry: p = [3, 4, 5], q = [4, 4, 4], ranks [32, 32] -- four pivot slices (values of i_1) per table, 16 lookups per chunk.  A
table's lookups are dealt onto its pivot slices by LENS: a slice of 17 lookups is a chunk of 16 and a chunk of 1, the others
are chunks of 4, 5, 1 and 16, and every table has one slice without a lookup.  With three tables the pivot slices are
s = table * 4 + i_1, so the kernel's quotient s / p_1 sees the tables 0, 1 and 2.  Six bags per table, one of them empty.

    python tests/entry_chain_cases.py --write-golden

runs every case on the GPU and records inputs and results under tests/golden/entry_chain_t<tables>.npz: indices, offsets,
weights, bag gradients and the forward outputs in full; the cores (regenerated from their seed by gen_inputs.make_cores), the
dense gradients and the cores after a fused SGD step as SHA-256 digests of their float32 bytes -- a bitwise comparison needs no
more, and the files stay a few KB.  The committed files were written by the commit BEFORE the entry chain was shortened
(the library is chosen with TTX_LIB): nothing arithmetic moved, so the kernels must give them back bit for bit."""
import hashlib
import os
import sys

import numpy as np

P, Q, R = [3, 4, 5], [4, 4, 4], [1, 32, 32, 1]
D, B, MC, LR = 64, 6, 16, 0.1
LENS = {1: [[17, 4, 5, 0]], 3: [[17, 4, 5, 0], [0, 1, 16, 5], [4, 17, 0, 1]]}   # lookups per (table, i_1)
SEED = {1: 9101, 3: 9103}
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sha(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(a.tobytes()).hexdigest()


def make_case(tables):
    """-> dict(indices, offsets, psw, d_out): deterministic, numpy's legacy generator"""
    import gen_inputs as G

    rs = np.random.RandomState(SEED[tables])
    idx, off = [], [0]
    for k in range(tables):
        i1 = np.repeat(np.arange(P[1]), LENS[tables][k])
        rs.shuffle(i1)
        n = i1.size
        i0, i2 = rs.randint(0, P[0], n), rs.randint(0, P[2], n)
        idx.append((i0 * P[1] + i1) * P[2] + i2)
        cuts = np.sort(rs.choice(np.arange(1, n), B - 2, replace=False))
        sizes = np.diff(np.concatenate([[0], cuts, [n]]))                 # B - 1 bags with lookups ...
        sizes = np.insert(sizes, rs.randint(0, B), 0)                     # ... and an empty one
        off += list(off[-1] + np.cumsum(sizes))
    idx = np.concatenate(idx).astype(np.int64)
    psw = (rs.rand(idx.size) + 0.5).astype(np.float32)
    return dict(indices=idx, offsets=np.array(off, dtype=np.int64), psw=psw, d_out=G.make_grad(SEED[tables] + 1, tables, B, D))


def make_cores(tables):
    import gen_inputs as G

    return G.make_cores(SEED[tables] + 2, tables, P, Q, R[1:-1])


def pivot_lengths(tables, indices, tableidx):
    """lookups per pivot slice s = table * p_1 + i_1"""
    i1 = (np.asarray(indices) // P[2]) % P[1]
    return np.bincount(np.asarray(tableidx) * P[1] + i1, minlength=tables * P[1]).reshape(tables, P[1])


def run(E, tables, case, cores, weighted, plan_rows, offsets=False):
    """forward, dense gradients, fused SGD step through one plan -> (out, [grads], [cores after the step]) as numpy float32.
    offsets: the forward is given the bags' offsets, so the contraction kernel pools the bags itself (the fused-pooling variant
    of spec_fwd_kernel, which finds a lookup's table from its pivot slice per lane) -- the same output bit for bit"""
    import torch

    import tt_ref64 as R64

    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rowidx, tableidx = R64.rowidx_from_offsets(case["offsets"], tables)
    nnz = int(case["indices"].size)
    ti, trow, ttab, d_out = t(case["indices"]), t(rowidx), t(tableidx), t(case["d_out"])
    w = t(case["psw"]) if weighted else None
    Lt = torch.zeros(3, dtype=torch.int64, device=dev)
    plan = E.make_plan(tables, P, Q, R, nnz, ti, ttab, rowidx=trow if plan_rows else None)
    dc = [t(c) for c in cores]
    out = E.tt_forward(1000, tables, B, D, P, Q, R, Lt, nnz, ti, trow, ttab, dc, plan=plan, per_sample_weights=w,
                       offsets=t(case["offsets"]) if offsets else None)
    grads = E.tt_dense_backward(1000, D, P, Q, R, Lt, nnz, ti, trow, ttab, d_out, dc, plan=plan, per_sample_weights=w)
    E.tt_sgd_backward(1000, D, LR, P, Q, R, Lt, nnz, ti, trow, ttab, d_out, dc, plan=plan, per_sample_weights=w)
    torch.cuda.synchronize()
    return out.cpu().numpy(), [g.cpu().numpy() for g in grads], [c.cpu().numpy() for c in dc]


def golden_path(tables):
    return os.path.join(GOLDEN, f"entry_chain_t{tables}.npz")


def write_golden():
    import tt_embeddings as E

    for tables in (1, 3):
        case, cores = make_case(tables), make_cores(tables)
        blob = dict(case)
        blob["cores_sha"] = np.array([sha(c) for c in cores])
        for weighted in (False, True):
            out, grads, new = run(E, tables, case, cores, weighted, True)
            out2, grads2, new2 = run(E, tables, case, cores, weighted, False)
            assert np.array_equal(out, out2) and all(np.array_equal(a, b) for a, b in zip(grads + new, grads2 + new2)), \
                "a plan with bag rows and one without disagree"
            k = f"w{int(weighted)}"
            blob[k + "_out"] = out
            blob[k + "_grad_sha"] = np.array([sha(g) for g in grads])
            blob[k + "_sgd_sha"] = np.array([sha(c) for c in new])
        np.savez_compressed(golden_path(tables), **blob)
        print("wrote", golden_path(tables), os.path.getsize(golden_path(tables)), "bytes")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [here, os.path.join(os.path.dirname(here), "fbtt-embedding_amd")]
    if "--write-golden" in sys.argv:
        write_golden()
