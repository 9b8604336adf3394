"""A float64 numpy restatement of TT-SVD and of the expansion of TT cores, for tests/test_svd_cpu.py and tests/test_svd_gpu.py.

TEST INFRASTRUCTURE ONLY.  Written from Oseledets 2011, Algorithm 1, with `np.linalg.svd` on the EXPLICIT unfoldings (no Gram
matrices, no chunks, nothing shared with fbtt-embedding_amd/ttx_svd.py) and an explicit entry-by-entry `tt_full`.  Every expected
number of the two test files comes from here, never from the code under test.

Canonical cores: core k is [r_k, p_k, q_k, r_{k+1}], r_0 = r_T = 1; table entry (i, j) = prod_k core_k[:, i_k, j_k, :] with
i = (i_0 .. i_{T-1}) in the row factors p, j = (j_0 .. j_{T-1}) in the column factors q, digit 0 the most significant.
"""
import itertools

import numpy as np


def tt_full(cores, num_embeddings=None):
    """the table [prod(p), prod(q)] of canonical cores, float64: one chain of small matrix products per (row, column) digit pair,
    written out entry block by entry block"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    p, q = [c.shape[1] for c in cores], [c.shape[2] for c in cores]
    P, D = int(np.prod(p)), int(np.prod(q))
    full = np.zeros((P, D))
    for i_digits in itertools.product(*[range(v) for v in p]):
        i = 0
        for d, v in zip(i_digits, p):
            i = i * v + d
        for j_digits in itertools.product(*[range(v) for v in q]):
            j = 0
            for d, v in zip(j_digits, q):
                j = j * v + d
            acc = np.ones((1, 1))
            for c, a, b in zip(cores, i_digits, j_digits):
                acc = acc @ c[:, a, b, :]
            full[i, j] = acc[0, 0]
    return full if num_embeddings is None else full[:num_embeddings]


def tensor_of(weight, p, q):
    """the table [E, D], rows zero-padded to prod(p), as the tensor [n_0 .. n_{T-1}] of modes n_k = p_k q_k (index i_k q_k + j_k)"""
    W = np.asarray(weight, dtype=np.float64)
    P, T = int(np.prod(p)), len(p)
    padded = np.zeros((P, W.shape[1]))
    padded[:W.shape[0]] = W
    t = padded.reshape(list(p) + list(q)).transpose([x for k in range(T) for x in (k, T + k)])
    return np.ascontiguousarray(t).reshape([a * b for a, b in zip(p, q)])


def tt_svd(weight, p, q, ranks=None, rel_error=None):
    """-> dict(cores: canonical float64 cores of the ranks KEPT (at most what an unfolding admits), ranks, eps_k, bound, norm,
    sigma: per step the singular values of the step's unfolding)"""
    assert (ranks is None) != (rel_error is None)
    T = len(p)
    modes = [a * b for a, b in zip(p, q)]
    C = tensor_of(weight, p, q)
    norm = float(np.sqrt((C * C).sum()))
    delta = None if rel_error is None else rel_error * norm / np.sqrt(T - 1)
    cores, kept, eps_k, sigma = [], [1], [], []
    C = C.reshape(modes[0], -1)
    for k in range(T - 1):
        U, S, Vt = np.linalg.svd(C, full_matrices=False)
        sigma.append(S)
        if ranks is not None:
            r = min(int(ranks[k]), S.size)
        else:
            r = 1
            while r < S.size and np.sqrt((S[r:] ** 2).sum()) > delta:
                r += 1
        eps_k.append(float(np.sqrt((S[r:] ** 2).sum())))
        cores.append(U[:, :r].reshape(kept[-1], p[k], q[k], r))
        kept.append(r)
        C = (S[:r, None] * Vt[:r]).reshape(r * modes[k + 1], -1)
    cores.append(C.reshape(kept[-1], p[-1], q[-1], 1))
    return dict(cores=cores, ranks=kept[1:], eps_k=eps_k, bound=float(np.sqrt(sum(e * e for e in eps_k))), norm=norm, sigma=sigma)


def error(weight, cores):
    """||W - tt_full(cores)||_F over ALL prod(p) rows (the rows past E are zero in W)"""
    cores = [np.asarray(c, dtype=np.float64) for c in cores]
    p, q = [c.shape[1] for c in cores], [c.shape[2] for c in cores]
    full = tt_full(cores)
    W = np.zeros_like(full)
    W[:np.asarray(weight).shape[0]] = np.asarray(weight, dtype=np.float64)
    return float(np.sqrt(((full - W) ** 2).sum()))


def unfolding_tails(weight, p, q, ranks):
    """per split k: the Eckart-Young tail sqrt(sum_{i >= r_{k+1}} sigma_i^2) of the unfolding [n_0 .. n_k, n_{k+1} .. n_{T-1}] of the
    padded table ITSELF -- no TT of those ranks is closer to the table than the largest of them"""
    t = tensor_of(weight, p, q)
    out, rows = [], 1
    for k in range(len(p) - 1):
        rows *= t.shape[k]
        S = np.linalg.svd(t.reshape(rows, -1), compute_uv=False)
        out.append(float(np.sqrt((S[int(ranks[k]):] ** 2).sum())))
    return out


def pad_ranks(cores, ranks):
    """the same table at larger ranks: every core in the leading block of a zero core"""
    new = [1] + [int(r) for r in ranks] + [1]
    out = []
    for k, c in enumerate(cores):
        z = np.zeros((new[k], c.shape[1], c.shape[2], new[k + 1]))
        z[:c.shape[0], :, :, :c.shape[3]] = c
        out.append(z)
    return out


def random_cores(rs, p, q, ranks, dtype=np.float32):
    """random canonical cores of exactly these ranks, entries N(0, 1) / sqrt(r_k): products of O(1) size"""
    r = [1] + list(ranks) + [1]
    return [(rs.standard_normal((r[k], p[k], q[k], r[k + 1])) / np.sqrt(r[k])).astype(dtype) for k in range(len(p))]


# the smallest shapes at which a swapped mode or digit order shows: all factors distinct
CASES = {
    "T3": dict(p=[3, 4, 5], q=[2, 3, 4], E=57, ranks=[4, 3]),           # padded rows, D = 24
    "T2": dict(p=[4, 6], q=[3, 5], E=23, ranks=[5]),                    # D = 15: D % 4 != 0
    "T4": dict(p=[2, 3, 4, 5], q=[2, 2, 3, 2], E=117, ranks=[3, 4, 3]),  # four cores
    "cap": dict(p=[5, 4, 3], q=[4, 2, 2], E=60, ranks=[32, 32]),        # ranks above what the unfoldings admit: zero-padded
}
