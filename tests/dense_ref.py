"""float64 numpy restatement of the dense member tables (include/ttx.h "dense member tables"): the forward in its three modes,
padding, per-sample weights, the per-row gradient G_r, the three updates and the gradient of the weights.  Written from the
contract, lookup by lookup; checked against torch's own F.embedding_bag / optimizers by tests/test_dense_tables_cpu.py."""
import numpy as np


def lookups(indices, offsets, row_base, B, padding=None):
    """-> (bag[n], row[n]) per position: bag -1 for a position no bag covers, row -1 at padding (a negative index, or the table's
    padding value); every other index is clamped into its table"""
    indices, offsets = np.asarray(indices, np.int64), np.asarray(offsets, np.int64)
    nnz, nb = indices.size, offsets.size - 1
    bag, row = np.full(nnz, -1, np.int64), np.full(nnz, -1, np.int64)
    for b in range(nb):
        s, e = min(max(int(offsets[b]), 0), nnz), min(max(int(offsets[b + 1]), 0), nnz)
        t = b // B
        base, E = int(row_base[t]), int(row_base[t + 1] - row_base[t])
        pad = -1 if padding is None or padding[t] is None else int(padding[t])
        for n in range(s, e):
            bag[n] = b
            i = int(indices[n])
            if i >= 0 and i != pad:
                row[n] = base + min(i, E - 1)
    return bag, row


def forward(weight, indices, offsets, row_base, B, mode="sum", padding=None, psw=None, dtype=np.float64):
    """-> (out [nb, D], live [nb] int, argmax [nb, D] int: the winning position, -1 without a live slot).  dtype: the precision of
    the sums -- float64 (the reference), or float32: a plain fp32 sum in index order, the yardstick of a widened comparison"""
    w = np.asarray(weight, dtype)
    nb, D = len(offsets) - 1, w.shape[1]
    bag, row = lookups(indices, offsets, row_base, B, padding)
    out, live, arg = np.zeros((nb, D), dtype), np.zeros(nb, np.int64), np.full((nb, D), -1, np.int64)
    for n in range(len(bag)):
        b = bag[n]
        if b < 0 or row[n] < 0:
            continue
        v = w[row[n]]
        live[b] += 1
        if mode == "max":
            win = (arg[b] < 0) | (v > out[b])  # strict >: the first position keeps a tie
            out[b] = np.where(win, v, out[b])
            arg[b] = np.where(win, n, arg[b])
        else:
            out[b] += v * dtype(1.0 if psw is None else np.asarray(psw).reshape(-1)[n])
    if mode == "mean":
        out /= np.maximum(live, 1)[:, None].astype(dtype)
    return out, live, arg


def row_grads(weight, indices, offsets, row_base, B, d_out, mode="sum", padding=None, psw=None, dtype=np.float64):
    """-> (G [R, D], touched [R] bool, d_psw [nnz] from `weight` as given), summed in index order in `dtype`"""
    w, d = np.asarray(weight, dtype), np.asarray(d_out, dtype).reshape(len(offsets) - 1, -1)
    bag, row = lookups(indices, offsets, row_base, B, padding)
    _, live, arg = forward(weight, indices, offsets, row_base, B, mode, padding, psw)
    G, touched, d_psw = np.zeros_like(w), np.zeros(w.shape[0], bool), np.zeros(len(bag), dtype)
    for n in range(len(bag)):
        b, r = bag[n], row[n]
        if b < 0 or r < 0:
            continue
        touched[r] = True
        if mode == "max":
            G[r] += np.where(arg[b] == n, d[b], dtype(0.0))
        elif mode == "mean":
            G[r] += d[b] / dtype(live[b])
        else:
            G[r] += d[b] * dtype(1.0 if psw is None else np.asarray(psw).reshape(-1)[n])
        d_psw[n] = d[b] @ w[r]
    return G, touched, d_psw


# ---- the same three, vectorised ------------------------------------------------------------------------------------------------
# The loop forms above are the definition.  The forms below restate them with array operations for batches beyond ~20 k lookups,
# and add every contribution in the SAME order (np.add.at applies its operands one after the other, in index order), so they are
# bit for bit equal to the loop forms in float64 and in float32 -- the "plain sum in index order" yardstick included, in every
# mode.  tests/test_dense_tables_cpu.py pins that on every case of tests/dense_cases.py below 20 k lookups.  They need what the
# kernels' bag search needs: offsets that, clamped into [0, nnz], do not decrease.
def lookups_vec(indices, offsets, row_base, B, padding=None):
    indices, offsets = np.asarray(indices, np.int64), np.asarray(offsets, np.int64)
    row_base = np.asarray(row_base, np.int64)
    nnz, nb = indices.size, offsets.size - 1
    cs = np.clip(offsets, 0, nnz)
    assert nb < 1 or (np.diff(cs) >= 0).all(), "lookups_vec: the clamped offsets must not decrease (use lookups)"
    n = np.arange(nnz, dtype=np.int64)
    if nb < 1:
        return np.full(nnz, -1, np.int64), np.full(nnz, -1, np.int64)
    b = np.searchsorted(cs, n, side="right") - 1  # the last b with offsets[b] <= n
    covered = (b >= 0) & (b < nb)
    covered &= n < cs[np.clip(b + 1, 0, nb)]
    bag = np.where(covered, b, -1)
    t = np.where(covered, b, 0) // max(int(B), 1)
    base, E = row_base[t], row_base[t + 1] - row_base[t]
    pad = np.full(len(row_base) - 1, -1, np.int64)
    if padding is not None:
        pad = np.asarray([-1 if v is None else int(v) for v in padding], np.int64)
    live = covered & (indices >= 0) & (indices != pad[t])
    row = np.where(live, base + np.minimum(indices, E - 1), -1)
    return bag, row


def forward_vec(weight, indices, offsets, row_base, B, mode="sum", padding=None, psw=None, dtype=np.float64):
    w = np.asarray(weight, dtype)
    nb, D = len(offsets) - 1, w.shape[1]
    bag, row = lookups_vec(indices, offsets, row_base, B, padding)
    n = np.flatnonzero((bag >= 0) & (row >= 0))
    b, v = bag[n], w[row[n]]
    out, arg = np.zeros((nb, D), dtype), np.full((nb, D), -1, np.int64)
    live = np.bincount(b, minlength=nb).astype(np.int64)
    if mode == "max":
        top = np.full((nb, D), -np.inf, dtype)
        np.maximum.at(top, b, v)
        first = np.full((nb, D), len(bag), np.int64)  # the first position that holds the bag's maximum (strict > in the loop form)
        np.minimum.at(first, b, np.where(v == top[b], n[:, None], len(bag)))
        has = (live > 0)[:, None]
        out, arg = np.where(has, top, dtype(0.0)), np.where(has, first, -1)
    else:
        x = np.ones(len(n), dtype) if psw is None else np.asarray(psw).reshape(-1)[n].astype(dtype)
        np.add.at(out, b, v * x[:, None])
    if mode == "mean":
        out /= np.maximum(live, 1)[:, None].astype(dtype)
    return out, live, arg


def row_grads_vec(weight, indices, offsets, row_base, B, d_out, mode="sum", padding=None, psw=None, dtype=np.float64):
    w, d = np.asarray(weight, dtype), np.asarray(d_out, dtype).reshape(len(offsets) - 1, -1)
    bag, row = lookups_vec(indices, offsets, row_base, B, padding)
    _, live, arg = forward_vec(weight, indices, offsets, row_base, B, mode, padding, psw)
    n = np.flatnonzero((bag >= 0) & (row >= 0))
    b, r = bag[n], row[n]
    G, touched, d_psw = np.zeros_like(w), np.zeros(w.shape[0], bool), np.zeros(len(bag), dtype)
    touched[r] = True
    if mode == "max":
        add = np.where(arg[b] == n[:, None], d[b], dtype(0.0))
    elif mode == "mean":
        add = d[b] / live[b].astype(dtype)[:, None]
    else:
        x = np.ones(len(n), dtype) if psw is None else np.asarray(psw).reshape(-1)[n].astype(dtype)
        add = d[b] * x[:, None]
    np.add.at(G, r, add)
    if len(n):  # (a stack of [1, D] @ [D, 1] products: the dot routine that `d[b] @ w[r]` calls, once per lookup)
        d_psw[n] = np.matmul(d[b][:, None, :], w[r][:, :, None]).reshape(-1)
    return G, touched, d_psw


def sgd(weight, G, touched, lr):
    w = np.asarray(weight, np.float64).copy()
    w[touched] -= lr * G[touched]
    return w


def adagrad(weight, state, G, touched, lr, eps):
    """element-wise: s += G^2; w -= lr G / (sqrt(s) + eps), touched rows only"""
    w, s = np.asarray(weight, np.float64).copy(), np.asarray(state, np.float64).copy()
    s[touched] += G[touched] ** 2
    w[touched] -= lr * G[touched] / (np.sqrt(s[touched]) + eps)
    return w, s


def rowwise_adagrad(weight, state, G, touched, lr, eps):
    """row-wise: s_r += mean_e(G_e^2); w -= lr G / (sqrt(s_r) + eps), touched rows only"""
    w, s = np.asarray(weight, np.float64).copy(), np.asarray(state, np.float64).copy()
    s[touched] += (G[touched] ** 2).mean(axis=1)
    w[touched] -= lr * G[touched] / (np.sqrt(s[touched]) + eps)[:, None]
    return w, s


def make_batch(seed, Es, B, max_len=5, empty=0.2, pad=None, tie_table=None, silent_table=None, long_bag=None):
    """ragged table-major bags over tables of cardinalities Es: about `empty` of the bags empty, table k's padding value pad[k]
    sprinkled in, bag 1 of table 0 padding only (when it has a padding value), and -- tie_table -- the same index twice in a bag;
    silent_table: a table whose bags are all empty; long_bag = (table, bag, slots): one bag of that many slots.
    -> (indices, offsets, psw)"""
    rs = np.random.RandomState(seed)
    idx, off = [], [0]
    for t, E in enumerate(Es):
        p = None if pad is None else pad[t]
        for b in range(B):
            L = int(rs.randint(1, max_len + 1))
            if empty > 0 and (t * B + b) % int(round(1 / empty)) == 3:  # (every fifth bag, at the default)
                L = 0
            if long_bag is not None and long_bag[:2] == (t, b):
                L = int(long_bag[2])
            if silent_table == t:
                L = 0
            bag = rs.randint(0, E, size=L).tolist()
            if p is not None and L > 1 and rs.rand() < 0.5:
                bag[int(rs.randint(L))] = p
            if p is not None and t == 0 and b == 1:
                bag = [p, p, p]
            if tie_table == t and b == 0:
                bag = [bag[0] if bag and bag[0] != p else (0 if p != 0 else min(1, E - 1))] * 2 + bag
            idx += bag
            off.append(len(idx))
    idx = np.asarray(idx, np.int64)
    return idx, np.asarray(off, np.int64), rs.uniform(0.5, 1.5, size=idx.size).astype(np.float32)
