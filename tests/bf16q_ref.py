"""Float64 reference and the error bound of the FOUR-core bf16 inference forward (include/ttx.h "bf16 inference forward, four
cores").  TEST INFRASTRUCTURE ONLY; the three-core helpers stay in tests/bf16_ref.py.

Inputs are the bf16 cores (float32 arrays holding bf16 values).  `rows64` is the float64 chain product

    row[a, b, (c, d)] = sum_k2 x_0[a, (b, k2)] M[k2, (c, d)],    x_0 = c_0 c_1 (over k1),    M = c_2 c_3 (over k3)

and its bound, element by element:

    2^-7 sum_k2 |x_0| |M|  +  (r1 + r2 + r3 + 3) 2^-24 sum_{k1, k2, k3} |c_0| |c_1| |c_2| |c_3|

Derivation (u = 2^-24; a product of two bf16 values has at most 16 significant bits: exact in fp32).
(a) x_0 and M are accumulated in fp32 over r1 and r3 exact products: |x_0_hat - x_0| <= r1 u sum_k1 |c_0| |c_1| and
    |M_hat - M| <= r3 u sum_k3 |c_2| |c_3|, to first order.
(b) Each is rounded ONCE to bf16, nearest even, 8-bit significand: x_0_bf = x_0_hat (1 + e1), M_bf = M_hat (1 + e2), |e| <= 2^-9.
    The product carries (1 + e1)(1 + e2) - 1, at most 2^-8 + 2^-18 in magnitude: times |x_0| |M| and summed over k2 this is the
    first term, stated as 2^-7 -- the factor of two the three-core bound (tests/bf16_ref.py) leaves for the second-order terms
    of (a) under (b).
(c) The last product multiplies two bf16 values (exact in fp32) and adds r2 of them in fp32: <= r2 u sum_k2 |x_0_bf| |M_bf|
    <= r2 u sum |c_0| |c_1| |c_2| |c_3| to first order.  (a) carried through it gives (r1 + r3) u of the same sum.  Together
    (r1 + r2 + r3) u, stated with three more units: one per product, as the three-core bound has one per product.
A pooled element follows bf16_ref.pool64: the rows' bounds plus len u sum |row|."""
import numpy as np

from bf16_ref import U24, pool64, to_bf16  # noqa: F401  (re-exported: the tests take them from here)

U7 = 2.0 ** -7

# the shapes the tests run: (q, ranks)
SHAPES = [([2, 2, 2, 2], [16, 16, 16]), ([4, 4, 4, 4], [32, 32, 32]), ([3, 5, 2, 5], [40, 33, 24]), ([4, 4, 4, 8], [64, 64, 64]),
          ([2, 4, 4, 4], [32, 64, 16])]


def slices(cores, p, q, r, indices, tableidx, base=None):
    """-> (A [n, q0, r1], B [n, r1, q1, r2], C [n, r2, q2, r3], Dm [n, r3, q3]) float64 of every lookup.  cores[t]: [tables, p_t,
    slice] (or, with `base` [tables][4] and per-table p [tables][4], the p_tables form [1, sum p, slice])."""
    tab = np.asarray(tableidx, dtype=np.int64)
    idx = np.maximum(np.asarray(indices, dtype=np.int64), 0)
    sid = [np.zeros(len(tab), dtype=np.int64) for _ in range(4)]
    for k in (range(len(p)) if base is not None else [None]):
        m = tab == k if base is not None else np.ones(len(tab), bool)
        pk = p[k] if base is not None else p
        rest = idx[m]
        for t in (3, 2, 1, 0):
            i = rest % pk[t] if t else np.minimum(rest, pk[0] - 1)
            rest = rest // pk[t]
            sid[t][m] = (base[k][t] if base is not None else tab[m] * pk[t]) + i
    flat = [np.asarray(c, dtype=np.float64).reshape(-1, c.shape[-1]) for c in cores]
    return (flat[0][sid[0]].reshape(-1, q[0], r[0]), flat[1][sid[1]].reshape(-1, r[0], q[1], r[1]),
            flat[2][sid[2]].reshape(-1, r[1], q[2], r[2]), flat[3][sid[3]].reshape(-1, r[2], q[3]))


def chain(A, B, C, Dm):
    """-> (x_0 [n, q0, q1, r2], M [n, r2, q2, q3], rows [n, q0, q1, q2, q3]) in the arrays' own dtype"""
    x0 = np.einsum("nak,nkbj->nabj", A, B)
    M = np.einsum("njck,nkd->njcd", C, Dm)
    return x0, M, np.einsum("nabj,njcd->nabcd", x0, M)


def rows64(A, B, C, Dm):
    """-> (rows [n, D] float64, bound [n, D] float64)"""
    n = A.shape[0]
    x0, M, rows = chain(A, B, C, Dm)
    t1 = np.einsum("nabj,njcd->nabcd", np.abs(x0), np.abs(M))
    t2 = chain(np.abs(A), np.abs(B), np.abs(C), np.abs(Dm))[2]
    bound = U7 * t1 + (A.shape[2] + C.shape[1] + C.shape[3] + 3) * U24 * t2
    return rows.reshape(n, -1), bound.reshape(n, -1)
