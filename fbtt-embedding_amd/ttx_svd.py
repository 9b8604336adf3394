"""TT-SVD of a dense table and TT rank rounding (Oseledets 2011, Algorithms 1 and 2) -- DESIGN.md 4.18; not in the reference.

What `from_pretrained` / `truncate_ranks` of the modules run.  Pure torch, on CPU and GPU tensors alike: the arithmetic runs on the
device the input lives on, in float64 (Gram matrices of the unfoldings through the BLAS, symmetric eigendecompositions and small
SVDs / QRs through the LAPACK of that device); the cores come back in float32 (`dtype=`).  A one-off per table, no per-step path.

CANONICAL cores: core k is a tensor [r_k, p_k, q_k, r_{k+1}] with r_0 = r_T = 1 -- entry (i, j) of the table, i = (i_0 .. i_{T-1})
in the row factors p and j = (j_0 .. j_{T-1}) in the column factors q (digit 0 the most significant of both), is the product of
the matrices core_k[:, i_k, j_k, :].  The modules store core k of one table as `canonical.permute(1, 0, 2, 3).reshape(p_k,
r_k * q_k * r_{k+1})` (`to_module_layout` / `from_module_layout`): the [1, 0, 2, 3] that `full_weight()` hands to
`tt_matrix_to_full`.
"""
import math
from typing import List, NamedTuple, Optional, Sequence

import torch

# an unfolding of at most this many elements is decomposed by torch.linalg.svd itself (cheaper than a Gram matrix and an
# eigendecomposition, and exact down to the smallest singular values); larger ones go through the Gram matrix of their smaller side
_SVD_DIRECT_MAX = 1 << 18
# float64 elements a chunk of a large unfolding may take while its Gram matrix / projection is accumulated (256 MiB)
_CHUNK_ELEMS = 1 << 25


class TTFactors(NamedTuple):
    """what tt_svd / tt_round return"""
    cores: List[torch.Tensor]  # canonical cores [r_k, p_k, q_k, r_{k+1}], float32 (`dtype=`), zero-padded to `ranks`
    ranks: List[int]           # the T - 1 inner ranks of `cores`
    eps_k: List[float]         # the Frobenius mass discarded by truncation step k (T - 1 entries)
    bound: float               # sqrt(sum eps_k^2) >= ||W - tt_full(cores)||_F (up to the rounding of `cores` to float32)
    norm: float                # ||W||_F


# --------------------------------------------------------------------------------------------------------------------- layout
def _check_cores(cores: Sequence[torch.Tensor]) -> List[int]:
    """canonical cores -> [r_0 .. r_T]; ValueError when they do not chain"""
    if not 2 <= len(cores) <= 4:
        raise ValueError(f"2, 3 or 4 TT cores, got {len(cores)}")
    for k, c in enumerate(cores):
        if not isinstance(c, torch.Tensor) or c.dim() != 4 or not c.is_floating_point():
            raise ValueError(f"core {k}: a floating-point tensor [r_k, p_k, q_k, r_k+1]")
    ranks = [int(c.size(0)) for c in cores] + [int(cores[-1].size(3))]
    if ranks[0] != 1 or ranks[-1] != 1 or any(int(c.size(3)) != ranks[k + 1] for k, c in enumerate(cores)):
        raise ValueError(f"the cores' ranks do not chain from 1 to 1: {[tuple(c.shape) for c in cores]}")
    return ranks


def to_module_layout(cores: Sequence[torch.Tensor]) -> List[torch.Tensor]:
    """canonical cores -> one table's slices as the modules store them: [p_k, r_k * q_k * r_{k+1}]"""
    _check_cores(cores)
    return [c.permute(1, 0, 2, 3).reshape(c.size(1), -1).contiguous() for c in cores]


def from_module_layout(mats: Sequence[torch.Tensor], tt_q_shapes: Sequence[int], tt_ranks: Sequence[int]) -> List[torch.Tensor]:
    """one table's slices [p_k, r_k * q_k * r_{k+1}] -> canonical cores (copies).  `tt_ranks`: the T - 1 inner ranks, or
    [1, .., 1] as the modules keep them"""
    T = len(mats)
    ranks = [int(r) for r in tt_ranks]
    if len(ranks) == T - 1:
        ranks = [1] + ranks + [1]
    if len(ranks) != T + 1 or len(tt_q_shapes) != T:
        raise ValueError(f"{T} cores need {T} column factors and {T - 1} ranks")
    out = []
    for k, m in enumerate(mats):
        shape = (int(m.size(0)), ranks[k], int(tt_q_shapes[k]), ranks[k + 1])
        if m.dim() != 2 or m.size(1) != shape[1] * shape[2] * shape[3]:
            raise ValueError(f"core {k}: expected [p, {shape[1] * shape[2] * shape[3]}], got {list(m.shape)}")
        out.append(m.reshape(shape).permute(1, 0, 2, 3).contiguous().clone())
    return out


def tt_full(cores: Sequence[torch.Tensor], num_embeddings: Optional[int] = None) -> torch.Tensor:
    """canonical cores -> the table [prod(p), prod(q)] (its first `num_embeddings` rows), in the cores' dtype.  For tests and
    small tables: the whole table is formed."""
    ranks = _check_cores(cores)
    p, q = [int(c.size(1)) for c in cores], [int(c.size(2)) for c in cores]
    acc = cores[0].contiguous()
    for k in range(1, len(cores)):
        acc = acc.reshape(-1, ranks[k]) @ cores[k].contiguous().reshape(ranks[k], -1)
    T = len(cores)
    acc = acc.reshape([d for pq in zip(p, q) for d in pq])
    full = acc.permute(list(range(0, 2 * T, 2)) + list(range(1, 2 * T, 2))).contiguous().reshape(math.prod(p), math.prod(q))
    return full if num_embeddings is None else full[:int(num_embeddings)]


def tt_pad_ranks(cores: Sequence[torch.Tensor], ranks: Sequence[int]) -> List[torch.Tensor]:
    """the same table at the (entry by entry not smaller) inner ranks `ranks`: every core in the leading block of a zero core"""
    old = _check_cores(cores)
    new = [1] + [int(r) for r in ranks] + [1]
    if len(new) != len(old) or any(a < b for a, b in zip(new, old)):
        raise ValueError(f"ranks {list(ranks)}: {len(old) - 2} ranks, none below the cores' {old[1:-1]}")
    if new == old:
        return [c.clone() for c in cores]
    out = []
    for k, c in enumerate(cores):
        z = c.new_zeros((new[k], c.size(1), c.size(2), new[k + 1]))
        z[:old[k], :, :, :old[k + 1]] = c
        out.append(z)
    return out


# ---------------------------------------------------------------------------------------------------------------- arguments
def _check_rank_args(T: int, ranks, rel_error, max_rank, rank_multiple, name: str) -> Optional[List[int]]:
    if (ranks is None) == (rel_error is None):
        raise ValueError(f"exactly one of {name} and rel_error must be given")
    if isinstance(rank_multiple, bool) or not hasattr(rank_multiple, "__index__") or int(rank_multiple) < 1:
        raise ValueError(f"rank_multiple must be a positive integer, got {rank_multiple!r}")
    if max_rank is not None and (isinstance(max_rank, bool) or not hasattr(max_rank, "__index__") or int(max_rank) < 1):
        raise ValueError(f"max_rank must be None or a positive integer, got {max_rank!r}")
    if rel_error is not None:
        if not 0.0 < float(rel_error) < 1.0:
            raise ValueError(f"rel_error must lie in (0, 1), got {rel_error!r}")
        return None
    ranks = [int(r) for r in ranks]
    if len(ranks) != T - 1:
        raise ValueError(f"{name}: {T} cores have {T - 1} inner ranks, got {len(ranks)}")
    if any(r < 1 for r in ranks):
        raise ValueError(f"{name} must be positive, got {ranks}")
    return ranks


# ---------------------------------------------------------------------------------------------------- one truncation step
def _chunks(size: int, other: int):
    step = max(1, _CHUNK_ELEMS // max(1, other))
    return [(a, min(size, a + step)) for a in range(0, size, step)]


def _gram(C: torch.Tensor, rows: bool) -> torch.Tensor:
    """C C^T (rows) or C^T C in float64, C taken in chunks along the other side: no float64 copy of a large C"""
    m, n = C.shape
    side = m if rows else n
    G = torch.zeros((side, side), dtype=torch.float64, device=C.device)
    for a, b in (_chunks(n, m) if rows else _chunks(m, n)):
        X = (C[:, a:b] if rows else C[a:b]).to(torch.float64)
        if rows:
            G.addmm_(X, X.t())
        else:
            G.addmm_(X.t(), X)
    return G


def _project(Ut: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """Ut [r, m] (float64) @ C [m, n] -> [r, n] float64, C taken in column chunks"""
    out = torch.empty((Ut.size(0), C.size(1)), dtype=torch.float64, device=C.device)
    for a, b in _chunks(C.size(1), C.size(0)):
        out[:, a:b] = Ut @ C[:, a:b].to(torch.float64)
    return out


def _times(C: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """C [m, n] @ V [n, r] (float64) -> [m, r] float64, C taken in row chunks"""
    out = torch.empty((C.size(0), V.size(1)), dtype=torch.float64, device=C.device)
    for a, b in _chunks(C.size(0), C.size(1)):
        out[a:b] = C[a:b].to(torch.float64) @ V
    return out


def _truncate(C: torch.Tensor, rank: Optional[int], delta: float, max_rank: Optional[int]):
    """One step of the sweep on the unfolding C [m, n]: -> (U [m, r] float64 with orthonormal columns spanning the r leading left
    singular vectors, U^T C [r, n] float64, r, the discarded mass sqrt(sum_{i >= r} sigma_i^2)).  `rank`: keep min(rank, m, n);
    None: the fewest whose discarded mass is at most `delta`, at most `max_rank`.  The singular pairs come from
    torch.linalg.svd for a small C, else from the Gram matrix of C's smaller side (eigh): never a matrix with both sides large."""
    m, n = C.shape
    V = None
    if m * n <= _SVD_DIRECT_MAX:
        U, S, _ = torch.linalg.svd(C.to(torch.float64), full_matrices=False)
        lam = S * S
    else:
        lam, Q = torch.linalg.eigh(_gram(C, rows=m <= n))
        lam, Q = lam.flip(0).clamp_(min=0.0), Q.flip(1)
        U, V = (Q, None) if m <= n else (None, Q)
    lam_h = lam.cpu()
    if rank is not None:
        r = min(int(rank), m, n)
    else:
        tail = torch.sqrt(torch.cumsum(lam_h.flip(0), 0).flip(0))  # tail[i] = sqrt(sum_{j >= i} lam_j): what keeping i of them discards
        r = max(1, int((tail > delta).sum().item()))
        if max_rank is not None:
            r = min(r, int(max_rank))
    if V is not None:
        # the larger side's vectors: an orthonormal basis of span(C V_r) by QR -- no division by a (possibly tiny) singular value
        U = torch.linalg.qr(_times(C, V[:, :r].contiguous()), mode="reduced")[0]
    U = U[:, :r].contiguous()
    return U, _project(U.t().contiguous(), C), r, float(torch.sqrt(lam_h[r:].sum()).item())


def _round_up(r: int, multiple: int) -> int:
    return -(-r // multiple) * multiple


def _finish(cores3, p, q, eff: List[int], want: Optional[List[int]], rank_multiple: int, eps_k, norm: float, dtype) -> TTFactors:
    """cores [r_k, n_k, r_{k+1}] of the ranks the sweep kept -> the result at the requested ranks (given ranks: exactly those;
    chosen ranks: rounded up to rank_multiple), the surplus zero"""
    ranks = list(want) if want is not None else [_round_up(r, int(rank_multiple)) for r in eff[1:-1]]
    cores = [c.reshape(eff[k], p[k], q[k], eff[k + 1]).to(dtype) for k, c in enumerate(cores3)]
    return TTFactors(tt_pad_ranks(cores, ranks), ranks, [float(e) for e in eps_k], math.sqrt(sum(e * e for e in eps_k)), norm)


def _sweep(first: torch.Tensor, modes: List[int], later, ranks, delta: float, max_rank):
    """the left-to-right truncation.  `first`: the unfolding [n_0, rest] of step 0; `later(k, carry)`: the unfolding
    [r_k n_k, rest] of step k >= 1 from the carry [r_k, ..] the step before left.  -> (cores [r_k, n_k, r_{k+1}], ranks kept, eps_k)"""
    T = len(modes)
    cores3, eff, eps_k = [], [1], []
    C = first
    for k in range(T - 1):
        U, carry, r, eps = _truncate(C, None if ranks is None else ranks[k], delta, max_rank)
        cores3.append(U.reshape(eff[k], modes[k], r))
        eff.append(r)
        eps_k.append(eps)
        C = later(k + 1, carry)
    cores3.append(C.to(torch.float64).reshape(eff[-1], modes[-1], 1))
    return cores3, eff + [1], eps_k


# ------------------------------------------------------------------------------------------------------------------ TT-SVD
def _scatter_rows(dst: torch.Tensor, src: torch.Tensor, p_rest: List[int], q: List[int]) -> None:
    """rows src [e, D] -> dst, a VIEW of the shape [p_a .. p_{T-1}, q_0 .. q_{T-1}] (p_rest = its row factors) of a zero tensor:
    whole slabs of the leading row factor at a time, the last partial slab by recursion -- the rows past e stay zero"""
    stride = math.prod(p_rest[1:])
    whole = src.size(0) // stride
    if whole:
        dst[:whole].copy_(src[:whole * stride].reshape([whole] + p_rest[1:] + q))
    if src.size(0) - whole * stride:
        _scatter_rows(dst[whole], src[whole * stride:], p_rest[1:], q)


def tt_svd(weight: torch.Tensor, tt_p_shapes: Sequence[int], tt_q_shapes: Sequence[int], tt_ranks: Optional[Sequence[int]] = None,
           *, rel_error: Optional[float] = None, max_rank: Optional[int] = None, rank_multiple: int = 1,
           dtype: torch.dtype = torch.float32) -> TTFactors:
    """TT-SVD of the table `weight` [E, D] in the row factors `tt_p_shapes` (prod >= E; the rows past E are zero) and the column
    factors `tt_q_shapes` (prod == D), T = 2, 3 or 4 cores.

    `tt_ranks`: the result has exactly these inner ranks; a rank above what its unfolding admits (min(r_{k-1} n_{k-1},
    n_k .. n_{T-1}), n_k = p_k q_k) is filled with zeros, not reduced.  `rel_error=eps` instead: step k keeps the fewest singular
    values whose discarded mass is at most eps ||W||_F / sqrt(T - 1) -- so ||W - TT||_F <= eps ||W||_F --, at most `max_rank` of
    them (the guarantee then no longer holds: see `bound`), the ranks rounded up to `rank_multiple` with zeros.
    One copy of the table (in its own dtype, modes interleaved) is the transient memory; the Gram matrix of the first unfolding is
    accumulated over chunks of it in float64."""
    if not isinstance(weight, torch.Tensor) or weight.dim() != 2 or not weight.is_floating_point():
        raise ValueError("weight: a 2-D floating-point tensor [num_embeddings, embedding_dim]")
    p, q = [int(x) for x in tt_p_shapes], [int(x) for x in tt_q_shapes]
    T = len(p)
    if not 2 <= T <= 4 or len(q) != T or any(v < 1 for v in p + q):
        raise ValueError(f"2, 3 or 4 positive row factors and as many column factors, got {p} and {q}")
    E, D = int(weight.size(0)), int(weight.size(1))
    if math.prod(q) != D:
        raise ValueError(f"prod(tt_q_shapes) = {math.prod(q)} is not the embedding dimension {D}")
    if math.prod(p) < E:
        raise ValueError(f"prod(tt_p_shapes) = {math.prod(p)} is below the {E} rows of the table")
    ranks = _check_rank_args(T, tt_ranks, rel_error, max_rank, rank_multiple, "tt_ranks")
    with torch.no_grad():
        weight = weight.detach()
        norm = math.sqrt(sum(float(weight[a:b].to(torch.float64).square().sum().item()) for a, b in _chunks(E, D)))
        delta = float(rel_error) * norm / math.sqrt(T - 1) if rel_error is not None else 0.0
        modes = [a * b for a, b in zip(p, q)]
        # the table with its modes interleaved [p_0, q_0, p_1, q_1, ..]: row digit i_0 and column digit j_0 the most significant
        inter = torch.zeros([d for pq in zip(p, q) for d in pq], dtype=weight.dtype, device=weight.device)
        _scatter_rows(inter.permute(list(range(0, 2 * T, 2)) + list(range(1, 2 * T, 2))), weight, p, q)

        def later(k, carry):  # [r_k, n_k .. n_{T-1}] -> [r_k n_k, n_{k+1} .. n_{T-1}]
            return carry.reshape(carry.size(0) * modes[k], -1)

        cores3, eff, eps_k = _sweep(inter.reshape(modes[0], -1), modes, later, ranks, delta, max_rank)
        del inter
        return _finish(cores3, p, q, eff, ranks, rank_multiple, eps_k, norm, dtype)


# ---------------------------------------------------------------------------------------------------------------- rounding
def tt_round(cores: Sequence[torch.Tensor], new_ranks: Optional[Sequence[int]] = None, *, rel_error: Optional[float] = None,
             max_rank: Optional[int] = None, rank_multiple: int = 1, dtype: torch.dtype = torch.float32) -> TTFactors:
    """TT rounding of canonical cores: a right-to-left QR orthogonalisation, then the left-to-right truncation of tt_svd on the
    small matrices [r_k n_k, r_{k+1}] -- the table is never formed.  `new_ranks` / `rel_error` / `max_rank` / `rank_multiple`: as
    tt_svd's; a `new_ranks[k]` at or above what core k carries leaves the table as it is (zero padding).  `norm` is the
    Frobenius norm of the table the cores stand for (all of its prod(p) rows)."""
    old = _check_cores(cores)
    T = len(cores)
    ranks = _check_rank_args(T, new_ranks, rel_error, max_rank, rank_multiple, "new_ranks")
    p, q = [int(c.size(1)) for c in cores], [int(c.size(2)) for c in cores]
    modes = [a * b for a, b in zip(p, q)]
    with torch.no_grad():
        G = [c.detach().to(torch.float64).reshape(old[k], modes[k], old[k + 1]) for k, c in enumerate(cores)]
        for k in range(T - 1, 0, -1):  # core k = R^T Q^T, rows of Q^T orthonormal; R^T goes into core k - 1
            Q, R = torch.linalg.qr(G[k].reshape(G[k].size(0), -1).t(), mode="reduced")
            G[k] = Q.t().reshape(Q.size(1), modes[k], -1)
            G[k - 1] = (G[k - 1].reshape(-1, G[k - 1].size(2)) @ R.t()).reshape(G[k - 1].size(0), modes[k - 1], -1)
        norm = float(torch.linalg.vector_norm(G[0]).item())
        delta = float(rel_error) * norm / math.sqrt(T - 1) if rel_error is not None else 0.0

        def later(k, carry):  # [r_k, r'_k] (what the truncation left of core k - 1) into core k -> [r_k n_k, r_{k+1}]
            return (carry @ G[k].reshape(G[k].size(0), -1)).reshape(carry.size(0) * modes[k], -1)

        cores3, eff, eps_k = _sweep(G[0].reshape(modes[0], -1), modes, later, ranks, delta, max_rank)
        return _finish(cores3, p, q, eff, ranks, rank_multiple, eps_k, norm, dtype)


def merged_ranks(results: Sequence[TTFactors]) -> List[int]:
    """the per-position maximum of several tables' ranks: what one batched module of them is built at"""
    return [max(r.ranks[k] for r in results) for k in range(len(results[0].ranks))]
