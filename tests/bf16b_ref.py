"""Float64 reference and the error bound of the pooled one-launch bf16 forward (include/ttx.h "bf16 inference forward, pooled in one
launch").  TEST INFRASTRUCTURE ONLY.
A bag is ONE fp32 accumulation chain per wave over its live lookups and their k2, plus a four-way combine (not bf16_ref.pool64's
sum of rows).  With w_l the weights (1 without), live the bag's lookups that are not padding, L = ceil(live / 4), per element:
    2^-8 sum_l |w_l| sum_k2 |x_0| |c_2|  +  (r1 + L r2 + 6) 2^-24 sum_l |w_l| sum_{k1, k2} |c_0| |c_1| |c_2|
First term: x_0 w is rounded once to bf16 (relative error <= 2^-9, stated as 2^-8 as in bf16_ref).  Second: r1 for the fp32
accumulation of x_0, L r2 for a chain of L r2 multiply-adds in any association, 1 for the weight, 3 for the combine of four partial
sums, 2 of slack.  mean: both over max(1, live), plus 2^-24 |out| for the division."""
import numpy as np

import bf16_ref as R


def bags64(cores, p, q, r, tables, idx, off, weights=None, padding_idx=None, mean=False):
    """-> (pooled [nb, D] float64, its bound); bag b belongs to table b // (nb // tables)"""
    nb = len(off) - 1
    tab = np.repeat(np.arange(nb) // (nb // tables), np.diff(off))
    A, B, C = R.slices(cores, p, q, r, idx, tab)
    x0 = np.einsum("nak,nkbj->nabj", A, B)
    rows = np.einsum("nabj,njc->nabc", x0, C).reshape(len(idx), -1)
    t1 = np.einsum("nabj,njc->nabc", np.abs(x0), np.abs(C)).reshape(rows.shape)
    t2 = np.einsum("nabj,njc->nabc", np.einsum("nak,nkbj->nabj", np.abs(A), np.abs(B)), np.abs(C)).reshape(rows.shape)
    keep = np.ones(len(idx), bool) if padding_idx is None else np.asarray(idx) != padding_idx
    w = (np.ones(len(idx)) if weights is None else np.asarray(weights, np.float64)) * keep
    out, bnd = np.zeros((nb, rows.shape[1])), np.zeros((nb, rows.shape[1]))
    for b in range(nb):
        s, e = int(off[b]), int(off[b + 1])
        live = int(keep[s:e].sum())
        aw = np.abs(w[s:e, None])
        out[b] = (w[s:e, None] * rows[s:e]).sum(0)
        bnd[b] = R.U8 * (aw * t1[s:e]).sum(0) + (r[0] + -(-live // 4) * r[1] + 6) * R.U24 * (aw * t2[s:e]).sum(0)
        if mean:
            out[b] /= max(1, live)
            bnd[b] = bnd[b] / max(1, live) + R.U24 * np.abs(out[b])
    return out, bnd
