"""Float64 reference and the error bound of the bf16 inference forward (include/ttx.h "bf16 inference forward").
TEST INFRASTRUCTURE ONLY.

Inputs are the bf16 cores (float32 arrays holding bf16 values).  `rows64` is the float64 chain product of a three-core table,

    row[a, b, c] = sum_k2 x_0[a, (b, k2)] c_2[k2, c],    x_0[a, (b, k2)] = sum_k1 c_0[a, k1] c_1[k1, (b, k2)]

and `bound` the derived bound of the contract, element by element:

    2^-8 sum_k2 |x_0| |c_2|  +  (r1 + r2 + 2) 2^-24 sum_{k1, k2} |c_0| |c_1| |c_2|

Derivation.  A product of two bf16 values has at most 16 significant bits: exact in fp32.  (a) x_0 is accumulated in fp32 over
r1 terms: |x_0_hat - x_0| <= r1 u sum_k1 |c_0| |c_1| to first order, u = 2^-24.  (b) An implementation may round x_0_hat once to
bf16: relative error <= 2^-9 (round to nearest, 8-bit significand), which the contract states as 2^-8 |x_0| to absorb the second
order terms of (a) -- the first term of the bound after the multiplication by |c_2| and the sum over k2.  (c) The second product
is r2 multiply-adds in fp32 (x_0_hat c_2 is not exact any more: one rounding per product, one per addition, or one per fused
multiply-add): <= (r2 + 1) u sum_k2 |x_0_hat| |c_2| <= (r2 + 1) u sum |c_0| |c_1| |c_2| to first order.  (a) carried through the
second product gives r1 u sum |c_0| |c_1| |c_2|.  Together (r1 + r2 + 1) u, stated with one more unit of slack.
A pooled element adds its rows in fp32: the sum of the rows' bounds plus len u sum |row|."""
import numpy as np
import torch

U24 = 2.0 ** -24
U8 = 2.0 ** -8

# the shapes the issue names: (q, ranks)
SHAPES = [([4, 4, 4], [32, 32]), ([4, 4, 8], [64, 64]), ([3, 4, 5], [13, 12]), ([2, 2, 4], [16, 16]), ([3, 3, 3], [8, 8])]


def to_bf16(x):
    """float32 array -> the float32 array of its bf16 roundings (torch's round to nearest even)"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def decode(indices, p):
    idx = np.maximum(np.asarray(indices, dtype=np.int64), 0)
    i2 = idx % p[2]
    i1 = (idx // p[2]) % p[1]
    i0 = np.minimum(idx // (p[1] * p[2]), p[0] - 1)
    return i0, i1, i2


def slices(cores, p, q, r, indices, tableidx, base=None):
    """-> (A [n, q0, r1], B [n, r1, q1, r2], C [n, r2, q2]) float64 of every lookup.  cores[t]: [tables, p_t, slice] (or, with
    `base` [tables][3] and per-table p [tables][3], the p_tables form [1, sum p, slice])."""
    tab = np.asarray(tableidx, dtype=np.int64)
    if base is None:
        i = decode(indices, p)
        sid = [tab * p[t] + i[t] for t in range(3)]
    else:
        sid = [np.zeros(len(tab), dtype=np.int64) for _ in range(3)]
        for k in range(len(p)):
            m = tab == k
            i = decode(np.asarray(indices)[m], p[k])
            for t in range(3):
                sid[t][m] = base[k][t] + i[t]
    flat = [np.asarray(c, dtype=np.float64).reshape(-1, c.shape[-1]) for c in cores]
    A = flat[0][sid[0]].reshape(-1, q[0], r[0])
    B = flat[1][sid[1]].reshape(-1, r[0], q[1], r[1])
    C = flat[2][sid[2]].reshape(-1, r[1], q[2])
    return A, B, C


def rows64(A, B, C):
    """-> (rows [n, D] float64, bound [n, D] float64)"""
    n = A.shape[0]
    r1, r2 = A.shape[2], C.shape[1]
    x0 = np.einsum("nak,nkbj->nabj", A, B)
    rows = np.einsum("nabj,njc->nabc", x0, C)
    t1 = np.einsum("nabj,njc->nabc", np.abs(x0), np.abs(C))
    t2 = np.einsum("nabj,njc->nabc", np.einsum("nak,nkbj->nabj", np.abs(A), np.abs(B)), np.abs(C))
    bound = U8 * t1 + (r1 + r2 + 2) * U24 * t2
    return rows.reshape(n, -1), bound.reshape(n, -1)


def pool64(rows, bound, offsets, mean=False):
    """-> (pooled [nb, D], its bound): the rows' bounds plus len 2^-24 sum |row| (mean: both over max(1, len), plus one rounding)"""
    nb = len(offsets) - 1
    out = np.zeros((nb, rows.shape[1]))
    bnd = np.zeros_like(out)
    for b in range(nb):
        s, e = int(offsets[b]), int(offsets[b + 1])
        out[b] = rows[s:e].sum(0)
        bnd[b] = bound[s:e].sum(0) + (e - s) * U24 * np.abs(rows[s:e]).sum(0)
        if mean:
            out[b] /= max(1, e - s)
            bnd[b] = bnd[b] / max(1, e - s) + U24 * np.abs(out[b])
    return out, bnd


def pool_f32_sequential(rows, offsets):
    """the float32 sum of each bag's rows in index order, starting from +0 (what ttx_bag_sum_pool computes, bit for bit)"""
    rows = np.asarray(rows, dtype=np.float32)
    nb = len(offsets) - 1
    out = np.zeros((nb, rows.shape[1]), dtype=np.float32)
    for b in range(nb):
        for j in range(int(offsets[b]), int(offsets[b + 1])):
            out[b] = out[b] + rows[j]
    return out
