"""A float64 reference of the TT path, written from the DEFINITION of the operation -- not from oracle/ttx_oracle.c (which it
checks) and not from any kernel.  TEST INFRASTRUCTURE: plain numpy.

The operation (table-batched, sum pooling).  A table of prod(p) rows of D = prod(q) floats is held as T cores; core t is
[tables, p_t, r_t * q_t * r_{t+1}] with r_0 = r_T = 1, a slice viewed as G_t[i_t] = [r_t, q_t, r_{t+1}].  Row `idx` has the digits
(i_0, .., i_{T-1}) of idx in the mixed radix p, MOST significant first, and is the chain product

    row[j_0, .., j_{T-1}] = G_0[i_0][:, j_0, :] @ G_1[i_1][:, j_1, :] @ .. @ G_{T-1}[i_{T-1}][:, j_{T-1}, :]        (a 1 x 1 matrix)

flattened with j_0 most significant.  out[table, bag] = sum of the rows of the bag's lookups (each times its per_sample_weight,
when weights are given).  The gradient of a loss with
d loss / d out = d_out with respect to G_t[i_t][a, j, b] is, summed over the lookups that use slice i_t of that table,

    sum_{l, m} Left_t[l, a] * g[l, j, m] * Right_t[b, m]

with Left_t = the product of the cores in front of t ([q_0 .. q_{t-1}, r_t]), Right_t = the product of the cores behind it
([r_{t+1}, q_{t+1} .. q_{T-1}]) and g = the bag's d_out row viewed as [q_0 .. q_{t-1}, q_t, q_{t+1} .. q_{T-1}].

Speed: a lookup's row and its slice gradients are linear in the bag gradient, so the lookups are grouped by DISTINCT (table, index)
-- each distinct pair is contracted once, with the sum of its lookups' bag gradients -- and the distinct pairs go through batched
`matmul` in blocks (a slice gradient is r q r doubles per core and pair).

Tables of different row factors (`p` a list of T-lists, one per table): the cores are [1, sum_k p_t(k), slice], table k's slices
behind those of the tables in front of it -- the library's layout (include/ttx.h, ttx_geom::p_tables)."""
import numpy as np

from util import record_wide_bounds


def _pad_ranks(r, T):
    r = [int(x) for x in r]
    return r if len(r) == T + 1 else [1] + r + [1]


class Geometry:
    """slice ids and extents of a (possibly mixed) table-batched TT geometry"""

    def __init__(self, tables, p, q, r):
        self.tables = int(tables)
        self.q = [int(x) for x in q]
        self.T = len(self.q)
        self.r = _pad_ranks(r, self.T)
        self.mixed = isinstance(p[0], (list, tuple, np.ndarray))
        pt = np.array(p if self.mixed else [list(p)] * self.tables, dtype=np.int64)  # [tables, T]
        assert pt.shape == (self.tables, self.T)
        self.p_tables = pt
        self.slice = [self.r[t] * self.q[t] * self.r[t + 1] for t in range(self.T)]
        self.S = [int(pt[:, t].sum()) for t in range(self.T)]                          # slices per core, all tables
        self.base = [np.concatenate([[0], np.cumsum(pt[:, t])[:-1]]) for t in range(self.T)]  # first slice of a table
        self.D = int(np.prod(self.q))

    def slice_ids(self, indices, tableidx):
        """-> [T] arrays of slice ids (rows of the cores' [S_t, slice] view), digits most significant first"""
        idx = np.asarray(indices, dtype=np.int64)
        tb = np.asarray(tableidx, dtype=np.int64)
        pt = self.p_tables[tb]                                                        # [nnz, T]
        assert (idx >= 0).all() and (idx < np.prod(pt, axis=1)).all(), "index out of its table's range"
        out, rem = [None] * self.T, idx.copy()
        for t in range(self.T - 1, -1, -1):
            out[t] = self.base[t][tb] + rem % pt[:, t]
            rem //= pt[:, t]
        return out

    def cores2d(self, cores, dtype=np.float64):
        out = []
        for t, c in enumerate(cores):
            c = np.asarray(c)
            assert c.size == self.S[t] * self.slice[t], f"core {t}: {c.shape} for {self.S[t]} slices of {self.slice[t]}"
            out.append(c.reshape(self.S[t], self.slice[t]).astype(dtype))
        return out


def rowidx_from_offsets(offsets, tables):
    """bags are table-major: bag b of table k is bag k * B + b -> (rowidx, tableidx) per lookup"""
    offsets = np.asarray(offsets, dtype=np.int64)
    nb = offsets.size - 1
    B = nb // tables
    bag = np.repeat(np.arange(nb, dtype=np.int64), np.diff(offsets))
    return bag % B, bag // B


def forward_backward(tables, p, q, r, B, indices, rowidx, tableidx, cores, d_out=None, block_doubles=1 << 23, per_sample_weights=None):
    """-> dict(out [tables, B, D], grads [T] x [shape of the core] (d_out given), touched [T] x bool[S_t]); all float64

    per_sample_weights (nn.EmbeddingBag's, one per lookup): out[bag] += w_n row_n, a lookup brings w_n d_out[bag(n)] to its pair's
    gradient, and -- d_out given -- d_psw[n] = <d_out[bag(n)], row_n> joins the results.  `touched` does not look at the weights:
    a lookup of weight 0 still touches its slices, as in the kernels.  None: the statements below are the unweighted ones, the
    results bit for bit what they were before the argument existed (tests/test_tt_ref64_cpu.py holds the earlier text against it)."""
    g = Geometry(tables, p, q, r)
    T, rr, qq = g.T, g.r, g.q
    idx = np.asarray(indices, dtype=np.int64)
    row = np.asarray(rowidx, dtype=np.int64)
    tb = np.asarray(tableidx, dtype=np.int64)
    nnz = idx.size
    psw = None if per_sample_weights is None else np.asarray(per_sample_weights, dtype=np.float64).reshape(-1)
    assert psw is None or psw.size == nnz, "one weight per lookup"
    W = g.cores2d(cores)
    out = np.zeros((tables * B, g.D))
    grads = [np.zeros_like(w) for w in W] if d_out is not None else None
    touched = [np.zeros(g.S[t], dtype=bool) for t in range(T)]
    res = dict(out=out.reshape(tables, B, g.D), touched=touched)
    if d_out is not None:
        res["grads"] = [gr.reshape(np.asarray(c).shape) for gr, c in zip(grads, cores)]
        if psw is not None:
            res["d_psw"] = np.zeros(nnz)
    if nnz == 0:
        return res
    sid = g.slice_ids(idx, tb)
    for t in range(T):
        touched[t][sid[t]] = True
    bag = tb * B + row
    # distinct (table, index) pairs; `inv` maps a lookup onto its pair
    emax = int(np.prod(g.p_tables, axis=1).max())
    key, first, inv = np.unique(tb * emax + idx, return_index=True, return_inverse=True)
    U = key.size
    usid = [s[first] for s in sid]
    gU = None
    if d_out is not None:
        gU = np.zeros((U, g.D))
        gbag = np.asarray(d_out, dtype=np.float64).reshape(tables * B, g.D)[bag]
        np.add.at(gU, inv, gbag if psw is None else psw[:, None] * gbag)
    rows = np.empty((U, g.D))
    blk = max(1, int(block_doubles // max(max(g.slice), g.D)))
    for u0 in range(0, U, blk):
        u1 = min(U, u0 + blk)
        n = u1 - u0
        G = [W[t][usid[t][u0:u1]].reshape(n, rr[t], qq[t], rr[t + 1]) for t in range(T)]
        # Left[t]: [n, q_0 .. q_{t-1}, r_t]
        left = [np.ones((n, 1, 1))]
        for t in range(T):
            nxt = np.matmul(left[t], G[t].reshape(n, rr[t], qq[t] * rr[t + 1]))          # [n, Ql, q_t r_{t+1}]
            left.append(nxt.reshape(n, -1, rr[t + 1]))
        rows[u0:u1] = left[T].reshape(n, g.D)
        if d_out is None:
            continue
        # Right[t]: [n, r_{t+1}, q_{t+1} .. q_{T-1}]
        right = [None] * T
        right[T - 1] = np.ones((n, 1, 1))
        for t in range(T - 1, 0, -1):
            prv = np.matmul(G[t].reshape(n, rr[t] * qq[t], rr[t + 1]), right[t])        # [n, r_t q_t, Qr]
            right[t - 1] = prv.reshape(n, rr[t], -1)
        for t in range(T):
            Ql, Qr = left[t].shape[1], right[t].shape[2]
            gg = gU[u0:u1].reshape(n, Ql, qq[t] * Qr)
            a = np.matmul(left[t].transpose(0, 2, 1), gg).reshape(n, rr[t] * qq[t], Qr)   # [n, r_t q_t, Qr]
            dG = np.matmul(a, right[t].transpose(0, 2, 1)).reshape(n, g.slice[t])         # [n, r_t q_t r_{t+1}]
            s = usid[t][u0:u1]
            order = np.argsort(s, kind="stable")
            ss = s[order]
            starts = np.flatnonzero(np.concatenate([[True], ss[1:] != ss[:-1]]))
            grads[t][ss[starts]] += np.add.reduceat(dG[order], starts, axis=0)
    if psw is None:
        np.add.at(out, bag, rows[inv])
        return res
    np.add.at(out, bag, psw[:, None] * rows[inv])
    if d_out is not None:
        res["d_psw"][:] = np.einsum("nd,nd->n", gbag, rows[inv])
    return res


def per_lookup_restatement(tables, B, rowidx, tableidx, per_sample_weights, d_out=None):
    """A weighted batch restated for an UNWEIGHTED implementation (the fp32 oracle, whose C has no weight argument): one bag per
    lookup -- B' = nnz, rowidx' = arange(nnz), the tables as they were -- and, for the gradients, d_out'[table(n), n] =
    w_n d_out[table(n), row(n)] (fp32, one rounding per element; rows of other tables' lookups zero).  The gradients of the cores
    of the restated batch ARE the weighted batch's.  -> dict(B, rowidx, d_out [tables, nnz, D] float32 or None)"""
    row = np.asarray(rowidx, dtype=np.int64)
    tb = np.asarray(tableidx, dtype=np.int64)
    w = np.asarray(per_sample_weights, dtype=np.float32).reshape(-1)
    nnz = row.size
    assert w.size == nnz
    ar = np.arange(nnz, dtype=np.int64)
    d2 = None
    if d_out is not None:
        d_out = np.asarray(d_out, dtype=np.float32)
        d2 = np.zeros((tables, nnz, d_out.shape[-1]), dtype=np.float32)
        d2[tb, ar] = w[:, None] * d_out.reshape(tables, B, -1)[tb, row]
    return dict(B=nnz, rowidx=ar, d_out=d2)


def pool_per_lookup_fp32(tables, B, rowidx, tableidx, per_sample_weights, rows_out, d_out=None):
    """the other half of the restatement: `rows_out` [tables, nnz, D] is an unweighted fp32 forward of the one-bag-per-lookup batch
    (row n at [table(n), n]) -- or [nnz, D], the lookups' rows themselves.  -> (out [tables, B, D]: the fp32 weighted sum out[bag(n)] += w_n row_n, lookup after lookup;
    d_psw [nnz] = <d_out[bag(n)], row_n> in fp32, or None)"""
    row = np.asarray(rowidx, dtype=np.int64)
    tb = np.asarray(tableidx, dtype=np.int64)
    w = np.asarray(per_sample_weights, dtype=np.float32).reshape(-1)
    rows = np.asarray(rows_out, dtype=np.float32)
    if rows.ndim == 3:
        rows = rows[tb, np.arange(row.size)]
    assert rows.shape[0] == row.size
    out = np.zeros((tables * B, rows.shape[-1]), dtype=np.float32)
    np.add.at(out, tb * B + row, w[:, None] * rows)                      # (float32 throughout: unbuffered, in lookup order)
    d_psw = None
    if d_out is not None:
        d_psw = np.einsum("nd,nd->n", np.asarray(d_out, dtype=np.float32).reshape(tables, B, -1)[tb, row], rows)
    return out.reshape(tables, B, -1), d_psw


def sgd_step(cores, grads, lr):
    """w - lr g in float64 (an untouched slice has g = 0: unchanged)"""
    return [np.asarray(c, dtype=np.float64) - float(lr) * np.asarray(gk, dtype=np.float64) for c, gk in zip(cores, grads)]


def adagrad_step(cores, state0, grads, touched, lr, eps):
    """one Adagrad step from the state `state0` on the touched slices: s = s0 + g^2, w = w0 - lr g / (sqrt(s) + eps);
    untouched slices keep weights and state.  -> (cores, state), float64"""
    new_w, new_s = [], []
    for c, s0, gk, m in zip(cores, state0, grads, touched):
        shp = np.asarray(c).shape
        w = np.asarray(c, dtype=np.float64).reshape(m.size, -1).copy()
        s = np.asarray(s0, dtype=np.float64).reshape(m.size, -1).copy()
        gg = np.asarray(gk, dtype=np.float64).reshape(m.size, -1)
        s[m] = s[m] + gg[m] * gg[m]
        w[m] = w[m] - float(lr) * gg[m] / (np.sqrt(s[m]) + float(eps))
        new_w.append(w.reshape(shp))
        new_s.append(s.reshape(shp))
    return new_w, new_s


def slice_mask(touched, cores):
    """[T] x bool of the cores' shapes: True on the elements of touched slices"""
    return [np.broadcast_to(m[:, None], (m.size, np.asarray(c).size // m.size)).reshape(np.asarray(c).shape)
            for m, c in zip(touched, cores)]


def oracle_on_restatement(tables, p, q, r, B, indices, rowidx, tableidx, per_sample_weights, cores, d_out, lr):
    """the fp32 oracle (oracle/ttx_oracle.c) on the one-bag-per-lookup restatement of a weighted case -> (out, d_psw, dense
    gradients, cores after one SGD step).  Its rows are computed once per distinct (table, index) pair (a row depends on nothing
    else); the SGD step is one fp32 step along its gradients."""
    import oracle_lib as O

    idx, tb = np.asarray(indices, dtype=np.int64), np.asarray(tableidx, dtype=np.int64)
    g = O.make_geom(tables, p, q, r)
    D, nnz = int(np.prod(q)), idx.size
    _, first, inv = np.unique(tb * int(np.prod(np.asarray(p, dtype=np.int64))) + idx, return_index=True, return_inverse=True)
    ar = np.arange(first.size, dtype=np.int64)
    rows = O.tt_forward(g, first.size, D, idx[first], ar, tb[first], cores)[tb[first], ar][inv]
    out, d_psw = pool_per_lookup_fp32(tables, B, rowidx, tb, per_sample_weights, rows, d_out)
    rst = per_lookup_restatement(tables, B, rowidx, tb, per_sample_weights, d_out)
    grads = O.tt_backward(g, O.OPTIM_DENSE, nnz, D, 0, 0, idx, rst["rowidx"], tb, rst["d_out"], [np.array(x, copy=True) for x in cores])
    return out, d_psw, grads, [c - np.float32(lr) * gk for c, gk in zip(cores, grads)]


# ---- distances in units of the project's default bound -----------------------------------------------------------------------
def default_units(got, ref, rtol=1e-5, atol_scale=2e-6):
    """max |got - ref| / (atol_scale max|ref| + rtol |ref|): 1 = at the default bound of tests/util.py::assert_close"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if ref.size == 0:
        return 0.0
    bound = atol_scale * max(float(np.abs(ref).max()), 1e-30) + rtol * np.abs(ref)
    return float((np.abs(got - ref) / bound).max())


WIDEN_CAP = 5.0  # (5e-5, 1e-5) in units of the default bound


def widen_factor(oracle, ref):
    """how much wider than the default a comparison against float64 may be: 1, or twice the fp32 oracle's own distance from
    float64 on the same case when that is more than half a default bound, capped.  -> (factor, the oracle's distance)"""
    u = default_units(oracle, ref)
    return (1.0 if u <= 0.5 else min(2.0 * u, WIDEN_CAP)), u


# ---- which site of the fused backward applies the update to a slice ------------------------------------------------------------
# Mirrors of the library's constants (csrc/ttx_internal.h, csrc/ttx_tt.hip, csrc/ttx_plan.hip); tests/test_tt_ref64_cpu.py reads
# the sources and fails when one of them is retuned without this file.
SEG_THIN = 256         # TTX_SEG_THIN: a thin core's slice is hot at more than 2 SEG_THIN lookups
HOT_PIVOT = 16         # TTX_HOT_PIVOT: a pivot slice is hot at more than this many chunk partials
MAX_HOT_PIVOT = 8      # TTX_MAX_HOT_PIVOT: more hot pivot slices than this (count known to the plan) stay with their owners
SEG_PIVOT = 32         # kSegPivot
PACK_MIN_SLICES = 1024  # the pack condition: nslices >= 1024 ...
PACK_MAX_FLOATS = 256   # ... every slice at most 4 * kWave floats (and a multiple of 4)
PLAN_TINY_NNZ = 1024   # at most this many lookups: the tiny plan (hot counts unknown to the plan)
PLAN_ONE_DIGIT = 256   # every core at most this many slices: the one-pass plans, which COUNT the hot pivot slices
PLAN_UNITS_MAX_NNZ = 256 * 4096  # (kMbFuseU wave units of 4096: beyond, the multi-pass plan, which does not count them)

# the forward's pooling dispatch (csrc/ttx_tt.hip tt_forward_impl, csrc/ttx_tt_spec.inc spec_launch_fwd)
POOL_SPAN_MIN = 65536  # kPoolSpanMin: at most this many lookups pool in pool4_small_kernel / inside the specialised forward kernel
SPEC_MC32 = 16         # TTX_MC32: lookups per (sub-)chunk of the q = [4,4,4], ranks [32,32] kernels; a plan chunk longer than this is walked in sub-chunks


def pool_route(nnz, D, offsets_given, specialised, padded=False):
    """which kernel pools the bags of ttx_tt_forward_o (16-byte aligned buffers, as torch's allocator gives): "fused" (inside
    spec_fwd_kernel: offsets and counters given, a specialised unpadded shape, D % 4 == 0, a small batch), "pool4_small", "pool4"
    or "pool_scalar" (pool_kernel)"""
    if D % 4:
        return "pool_scalar"
    if nnz > POOL_SPAN_MIN:
        return "pool4"
    return "fused" if (offsets_given and specialised and not padded) else "pool4_small"


SITES = ("packed", "float4_owner", "scalar_owner", "pivot_columns", "pivot_owner_fallback", "thin_fold", "t4_apply23")


def classify_apply_sites(indices, tableidx, tables, p, q, r, mc, merged_last_cores=False):
    """Which apply site of ttx_tt_backward's reduce / apply step every TOUCHED slice takes, from the batch alone.

    mc: lookups per chunk of the pivot core (core 1), the library's (the plan header's / ttx_debug_tiles').
    merged_last_cores: a four-core geometry on the three-core kernels -- cores 2 and 3 are applied by t4_apply23_kernel, cores
    0 and 1 by reduce_apply as a two-core geometry.
    -> dict(cores=[per core {site: number of touched slices}], lens=[per core lookups per slice], rows=[per core partial rows per
    slice], hot=[per core bool per slice: the slice leaves its owner], over=[per core bool per slice: beyond the hot threshold, as the
    plan header counts them -- a slice of odd size is counted and still stays with its owner], pack=bool, pivot_count_known=bool, shared_segments=[per core: segments of the sorted
    order in which two hot slices meet])"""
    g = Geometry(tables, p, q, r)
    T = g.T
    idx = np.asarray(indices, dtype=np.int64)
    nnz = idx.size
    sid = g.slice_ids(idx, tableidx)
    lens = [np.bincount(sid[t], minlength=g.S[t]) for t in range(T)]
    ra_cores = [0, 1] if merged_last_cores else list(range(T))  # the cores reduce_apply_kernel sees
    assert not merged_last_cores or T == 4
    nslices = sum(g.S[t] for t in ra_cores)
    sl = [g.slice[t] for t in ra_cores]
    pack = (not merged_last_cores and max(sl) <= PACK_MAX_FLOATS and all(s % 4 == 0 for s in sl) and nslices >= PACK_MIN_SLICES)
    tiny = nnz <= PLAN_TINY_NNZ and int(np.prod(g.p_tables, axis=1).max()) <= 2 ** 32
    known = not tiny and max(g.S) <= PLAN_ONE_DIGIT and not g.mixed and nnz <= PLAN_UNITS_MAX_NNZ
    cores, rows_all, hot_all, over_all, shared = [], [], [], [], []
    for t in range(T):
        n = lens[t]
        rows = -(-n // int(mc)) if t == 1 else n.copy()
        c = dict.fromkeys(SITES, 0)
        hot = np.zeros(n.size, dtype=bool)
        over_all.append(rows > (HOT_PIVOT if t == 1 else 2 * SEG_THIN))  # (what the PLAN counts: whatever the slice size or the site)
        nshared = 0
        if t not in ra_cores:
            c["t4_apply23"] = int((n > 0).sum())
        elif g.slice[t] % 4:
            c["scalar_owner"] = int((n > 0).sum())  # (odd slice sizes stay with their single owner, hot or not)
        else:
            hot = rows > (HOT_PIVOT if t == 1 else 2 * SEG_THIN)
            nh = int(hot.sum())
            owner = "packed" if pack else "float4_owner"
            c[owner] = int(((n > 0) & ~hot).sum())
            if t == 1:
                if known and nh > MAX_HOT_PIVOT:
                    c["packed" if pack else "pivot_owner_fallback"] += nh
                else:
                    c["pivot_columns"] = nh
            else:
                c["thin_fold"] = nh
                off = np.concatenate([[0], np.cumsum(n)])
                for s in np.flatnonzero(hot)[:-1]:
                    nxt = s + 1 + int(np.argmax(n[s + 1:] > 0)) if (n[s + 1:] > 0).any() else -1
                    # the next slice with lookups is hot too and starts inside the segment this one ends in
                    if nxt >= 0 and hot[nxt] and off[s + 1] % SEG_THIN != 0:
                        nshared += 1
        cores.append(c)
        rows_all.append(rows)
        hot_all.append(hot)
        shared.append(nshared)
    return dict(cores=cores, lens=lens, rows=rows_all, hot=hot_all, over=over_all, pack=bool(pack), pivot_count_known=bool(known),
                shared_segments=shared)


# ---- a live Adagrad state, and the bound of the state after one step -------------------------------------------------------------
def live_state(grads64, touched, seed):
    """fp32 Adagrad state to start a step from, per core: every element distinct; within each slice about half the elements LARGE
    (4 .. 6 max g^2 of the core's float64 gradient: the step is dominated by the prior state) and half SMALL (1e-3 .. 1.5e-3 max g^2:
    dominated by the gradient); untouched slices carry state too (they must come back bit-identical); ONE touched slice per core
    starts at zero (the first step of a row).  -> ([T] float32 arrays, [T] ids of the zeroed slices)"""
    rs = np.random.RandomState(seed)
    out, zeroed = [], []
    for gk, m in zip(grads64, touched):
        gk = np.asarray(gk, dtype=np.float64)
        n = gk.size
        m2 = max(float((gk * gk).max()), 1e-12)
        frac = (rs.permutation(n) + 1.0) / (n + 1.0)                 # distinct, in (0, 1)
        large = rs.rand(n) < 0.5
        s = np.where(large, 4.0 * m2 * (1.0 + 0.5 * frac), 1e-3 * m2 * (1.0 + 0.5 * frac)).astype(np.float32)
        assert np.unique(s).size == n, "the state's elements are meant to be distinct"
        s = s.reshape(m.size, -1)
        z = int(np.flatnonzero(m)[rs.randint(0, int(m.sum()))]) if m.any() else -1
        if z >= 0:
            s[z] = 0.0
        zeroed.append(z)
        out.append(np.ascontiguousarray(s.reshape(gk.shape)))
    return out, zeroed


def assert_state_close(got, ref_state, ref_g, what="", scale=1.0, rtol=1e-5, atol_scale=2e-6):
    """The Adagrad state s = s0 + g^2 after one step: a gradient within its bound dg = scale (atol_scale max|g| + rtol |g|) moves
    s by at most 2 |g| dg + dg^2; two fp32 ulps of s on top (the rounding of g * g and of the sum)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref_state, dtype=np.float64)
    g = np.abs(np.asarray(ref_g, dtype=np.float64))
    assert got.shape == ref.shape == g.shape, f"{what}: shapes {got.shape} {ref.shape} {g.shape}"
    assert np.isfinite(got).all() and np.isfinite(ref).all(), f"{what}: non-finite values"
    dg = float(scale) * (atol_scale * max(float(g.max()) if g.size else 0.0, 1e-30) + rtol * g)
    ulps = 2.0 * np.spacing(ref.astype(np.float32)).astype(np.float64)
    tol = 2.0 * g * dg + dg * dg + ulps
    err = np.abs(got - ref)
    if scale > 1.0:  # (a widened comparison: into the report like assert_close's)
        d1 = dg / float(scale)
        record_wide_bounds(what, rtol * scale, atol_scale * scale, err, tol, 2.0 * g * d1 + d1 * d1 + ulps)
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} out of tolerance; worst at {i}: got {got[i]!r} ref {ref[i]!r} "
                             f"tol {tol[i]:.3e} |g| {g[i]:.3e}")
