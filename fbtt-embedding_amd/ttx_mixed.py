"""Tables of DIFFERENT cardinality behind one module.

The reference batches only tables of identical shape (`TableBatchedTTEmbeddingBag`
asserts one `num_embeddings` / one set of TT shapes, tt_embeddings_ops.py:424,
README.md:136-141), so a real DLRM -- 26 sparse features with 26 different
cardinalities -- needs 26 separate modules and 26 x the launches.  Here the tables
are grouped by their TT shape: every group is ONE `TableBatchedTTEmbeddingBag`
(one plan, one forward, one backward for all its tables), and the call form is
DLRM's: one (indices, offsets) pair per table in, one [B, D] per table out.
`fused=True` goes one step further: ONE batched lookup for all tables whatever
their row factors (`VarTableTTEmbeddingBag`, include/ttx.h `ttx_geom::p_tables`).
Measured (scripts/bench_mixed.py, 8 tables of 4 shapes, B=512 x 20 lookups, eager
fwd+bwd+SGD): one module per table 0.600 ms/step, grouped 0.506, fused 0.293.
`streams=True` puts every group on a HIP stream of its own; the eager step is
host-bound at these sizes and the stream switches cost what the overlap gives
(0.600 ms/step) -- it is there for large batches and captured graphs.

    emb = MixedTTEmbeddingBag([1460, 583, 10131227, ...], 64, tt_ranks=[32, 32])
    outs = emb(lS_i, lS_o)        # lists of per-table tensors -> list of [B, D]
"""
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

import tt_embeddings_ops as _ops
from tt_embeddings_ops import (POOLING_MODES, OptimType, TableBatchedTTEmbeddingBag, _normalise_padding_idx,
                               suggested_tt_shapes)
from ttx_dense import DenseTableBatchedEmbeddingBag, dense_table_flags, dense_table_groups


def merge_bags(indices: Sequence[torch.Tensor], offsets: Sequence[torch.Tensor],
               include_last_offset: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """per-table (indices, offsets) -> the table-major batched form of `TableBatchedTTEmbeddingBag`
    (offsets with num_tables * B + 1 entries).  Lengths come from tensor shapes: no device read-back."""
    assert len(indices) == len(offsets) and len(indices) > 0
    nb = {int(o.numel()) for o in offsets}
    if len(nb) != 1:
        raise ValueError(f"every table must describe the same number of bags, got offsets of {sorted(nb)} entries")
    if include_last_offset and nb.pop() < 1:
        raise ValueError("include_last_offset form: offsets needs at least the closing entry")
    if __debug__ and include_last_offset and not indices[0].is_cuda:  # (host tensors only: no device read-back)
        for idx, off in zip(indices, offsets):
            assert int(off[-1]) == idx.numel(), "closing offset must equal the number of indices of the table"
    parts, base = [], 0
    for idx, off in zip(indices, offsets):
        starts = off[:-1] if include_last_offset else off
        parts.append(starts + base if base else starts)
        base += int(idx.numel())
    parts.append(torch.full((1,), base, dtype=parts[0].dtype, device=parts[0].device))
    return torch.cat([i.reshape(-1) for i in indices]), torch.cat(parts)


class VarTableTTEmbeddingBag(TableBatchedTTEmbeddingBag):
    """`TableBatchedTTEmbeddingBag` for tables of DIFFERENT row factors (same q and ranks): one plan, one
    forward, one backward launch set for all of them (include/ttx.h `ttx_geom::p_tables`).  Core t is one
    Parameter [1, sum_k p_k_t, r_t q_t r_{t+1}] holding the tables' slices one table after the other
    (`table_rows(t)[k]` = table k's rows of it); forward takes the table-major batched form, like the parent,
    and returns [num_tables, B, D].  `use_cache=True`: ONE LFU row cache over all the tables, keyed by key_base[table] + index
     -- the hottest rows across tables of any cardinality behind one hash table and one launch set."""

    def __init__(self, num_embeddings: Sequence[int], embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[Sequence[Optional[List[int]]]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 device: Optional[torch.device] = None, include_last_offset: bool = True,
                 table_ranks: Optional[Sequence[List[int]]] = None, table_q: Optional[Sequence[List[int]]] = None,
                 mode: str = "sum", padding_idx: Optional[int] = None, use_cache: bool = False, cache_size: int = 0,
                 hashtbl_size: int = 0, deterministic_cache_update: Optional[bool] = None,
                 reference_exact_populate: bool = False, betas: Tuple[float, float] = (0.9, 0.999), weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False) -> None:
        """`betas`, `weight_decay`, `decoupled_weight_decay` (trailing keywords, as on the parent): read under
        optimizer=OptimType.EXACT_ADAM only -- one fused Adam / AdamW step on all cores per backward; not with use_cache=True.
        `use_cache`, `cache_size`, `hashtbl_size`, `deterministic_cache_update`, `reference_exact_populate` (trailing keywords, as
        on the parent): ONE LFU row cache over all the tables, keyed by key_base[table] + index with key_base the
        running sum of the tables' prod(p) (`_key_space`).  Same buffers, parameters and state_dict() keys as the one-table cached
        module; defaults cache_size = int(0.1 * sum_k E_k), hashtbl_size = sum_k E_k.  Warm-up counts the batch's keys in one
        extra launch and runs the uncached routes; after cache_populate() the live route of the parent's table cache runs on the
        per-table row factors (TTTablesCachedLookupFunction).  Three cores only, no `table_q`, no mode="max"; GPU tensors once live.
        `mode`, `padding_idx` (trailing keywords, as on the parent): nn.EmbeddingBag's pooling modes and padded batches, on the
        parent's routes -- forward also takes the 2-D form `indices[num_tables * B, L]` with `offsets=None`.  `padding_idx` is ONE
        value for all tables, so it has to be a row of every one of them: torch's rule against the smallest cardinality.
        `table_q` (one factoring per table, entry by entry <= `tt_q_shapes`, every one a factoring of `embedding_dim`; round 4):
        tables whose output rows are factored DIFFERENTLY ride in the same batched lookup.  `tt_q_shapes` is then the common
        (padded) factoring the kernels run -- prod(tt_q_shapes) >= embedding_dim values per padded output row -- table k's cores are
        stored zero-padded to it like the ranks below, and forward() gathers every table's own embedding_dim values out of its
        padded rows (one gather launch; its backward scatters the gradient into zeros, so the padding's gradient is zero and the
        padding stays zero).
        `table_ranks` (one list per table, every entry <= the matching `tt_ranks` entry): tables of SMALLER TT ranks ride in the
        same batched lookup -- table k is initialised as a table of its own ranks and its slices are stored zero-padded to the
        common ranks.  The padding stays zero under the fused optimizers (every gradient term of a padded entry has a zero factor),
        so table k keeps behaving as a rank-`table_ranks[k]` table; what it costs is the multiply-adds on the zeros."""
        nn.Module.__init__(self)
        if mode not in POOLING_MODES:
            raise ValueError(f"mode must be one of {POOLING_MODES}, got {mode!r}")
        self.mode = mode
        self.padding_idx = _normalise_padding_idx(padding_idx, min(int(e) for e in num_embeddings))
        self.include_last_offset = bool(include_last_offset)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("VarTableTTEmbeddingBag needs a GPU")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        nd = len(tt_ranks) + 1
        if mode == "max" and nd != 3:
            # (max runs ttx_tt_rows_p / ttx_tt_backward_rows on a plan with per-table row factors; the two- and four-core routes
            #  of those two have never run on such a plan)
            raise NotImplementedError(f"mode='max' on tables of different row factors needs three TT cores, got {nd} "
                                      "(two- and four-core geometries: not offered)")
        Es = [int(e) for e in num_embeddings]
        assert len(Es) >= 1 and all(e > 0 for e in Es)
        ps = []
        for k, e in enumerate(Es):
            given = tt_p_shapes[k] if tt_p_shapes is not None else None
            ps.append([int(x) for x in given] if given is not None else suggested_tt_shapes(e, nd))
            assert len(ps[-1]) == nd and int(np.prod(np.asarray(ps[-1], dtype=np.int64))) >= e
        self.tt_q_shapes = [int(x) for x in tt_q_shapes] if tt_q_shapes is not None \
            else suggested_tt_shapes(int(embedding_dim), nd, allow_round_up=not enforce_embedding_dim)
        self.table_q = None if table_q is None else [[int(x) for x in q] for q in table_q]
        self.out_dim = int(embedding_dim)  # what forward() returns per bag
        if self.table_q is None:
            assert int(np.prod(self.tt_q_shapes)) == int(embedding_dim)
        else:
            assert tt_q_shapes is not None and len(self.table_q) == len(Es), "table_q: with the common tt_q_shapes, one per table"
            assert all(len(q) == nd and int(np.prod(q)) == self.out_dim and all(a <= b for a, b in zip(q, self.tt_q_shapes))
                       for q in self.table_q), "table_q: per table a factoring of embedding_dim, entry by entry <= tt_q_shapes"
        self.deterministic_cache_update = deterministic_cache_update
        self.reference_exact_populate = bool(reference_exact_populate)
        if use_cache:
            # the limits of the row cache over tables of different row factors, by name and before anything is built
            if mode == "max":
                raise NotImplementedError("mode='max' does not support use_cache=True (the cache rows are pooled by sum)")
            if nd != 3:
                # (the populate decompresses rows with ttx_tt_rows on a plan with per-table row factors, which has only ever run
                #  with three cores: ttx_cache_populate_v returns TTX_EUNSUPPORTED for any other count)
                raise NotImplementedError(f"use_cache=True on tables of different row factors needs three TT cores, got {nd}")
            if self.table_q is not None:
                raise NotImplementedError("use_cache=True does not support table_q: the cache rows would have the padded row "
                                          "length, over which row-wise Adagrad would average")
            cache_size = int(cache_size) if cache_size > 0 else int(0.1 * sum(Es))
            hashtbl_size = int(hashtbl_size) if hashtbl_size > 0 else sum(Es)
            if hashtbl_size >= 2 ** 31:
                raise ValueError(f"hashtbl_size must stay below 2^31, got {hashtbl_size} (the default is the sum of the tables' "
                                 f"num_embeddings: pass a smaller hashtbl_size)")
            space = sum(int(np.prod(np.asarray(p, dtype=object))) for p in ps)
            if space >= 2 ** 62:
                raise ValueError(f"the cache's key space sum_k prod(tt_p_shapes[k]) = {space} does not fit 2^62")
            assert hashtbl_size >= cache_size
        self.num_tables, self.tt_ndim = len(Es), nd
        # (the parent's forward sizes its output rows by embedding_dim: the PADDED row length when the factorings differ)
        self.table_num_embeddings, self.embedding_dim = Es, int(np.prod(self.tt_q_shapes))
        self.num_embeddings = max(Es)
        self.tt_ranks = [1] + [int(x) for x in tt_ranks] + [1]
        self.tt_p_shapes = ps                                  # one list per table (the ctypes route)
        self._p_flat = [v for row in ps for v in row]          # ... flattened for the C++ node
        self.sparse, self.optimizer, self.learning_rate, self.eps = sparse, optimizer, learning_rate, eps
        self.register_buffer("L", torch.zeros(nd, dtype=torch.int64, device=device))  # (strides are per table)
        from tt_embeddings_ops import _SGD_LIKE, BufferList
        self.tt_cores = nn.ParameterList()
        self.optimizer_state = BufferList("optimizer_state")
        stateful = optimizer not in _SGD_LIKE and (sparse or optimizer != OptimType.EXACT_ADAM)  # (Adam's state: with sparse=True only)
        for t in range(nd):
            shape = (1, sum(p[t] for p in ps), self.tt_ranks[t] * self.tt_q_shapes[t] * self.tt_ranks[t + 1])
            self.tt_cores.append(nn.Parameter(torch.empty(shape, device=device, dtype=torch.float32)))
            self.optimizer_state.append(torch.zeros(shape if stateful else 0, device=device, dtype=torch.float32))
        self._init_adam(betas, weight_decay, decoupled_weight_decay, use_cache)
        # every table is initialised as a table of its own cardinality would be
        self.table_ranks = None if table_ranks is None else [[1] + [int(x) for x in rk] + [1] for rk in table_ranks]
        if self.table_ranks is not None:
            assert len(self.table_ranks) == len(Es) and all(len(rk) == nd + 1 and all(a <= b for a, b in zip(rk, self.tt_ranks))
                                                             for rk in self.table_ranks), "table_ranks: per table, <= tt_ranks"
        for k, e in enumerate(Es):
            rk = self.tt_ranks if self.table_ranks is None else self.table_ranks[k]
            one = TableBatchedTTEmbeddingBag.__new__(TableBatchedTTEmbeddingBag)
            nn.Module.__init__(one)
            qk = self.tt_q_shapes if self.table_q is None else self.table_q[k]
            one.num_tables, one.tt_ndim, one.num_embeddings, one.embedding_dim = 1, nd, e, self.out_dim
            one.tt_ranks, one.tt_p_shapes, one.tt_q_shapes = rk, ps[k], qk
            one.tt_cores = [torch.empty((1, ps[k][t], rk[t] * qk[t] * rk[t + 1]), device=device) for t in range(nd)]
            TableBatchedTTEmbeddingBag.reset_parameters(one, weight_dist)
            with torch.no_grad():
                for t in range(nd):
                    self.set_table_core(k, t, one.tt_cores[t][0])
        if self.table_q is not None:  # column k, j: where value j of table k's output row sits in its padded row
            cols = []
            for q in self.table_q:
                at = np.zeros(q, dtype=np.int64)
                for t in range(nd):
                    shape = [1] * nd
                    shape[t] = q[t]
                    at += np.arange(q[t], dtype=np.int64).reshape(shape) * int(np.prod(self.tt_q_shapes[t + 1:]))
                cols.append(at.reshape(-1))
            self.register_buffer("_cols", torch.from_numpy(np.stack(cols)).to(device), persistent=False)
        self.use_cache = bool(use_cache)
        if use_cache:  # (one set for all tables; names, order and shapes as the one-table cached module registers them)
            self.register_buffer("hashtbl", torch.full((hashtbl_size,), -1, device=device, dtype=torch.int64))
            self.register_buffer("cache_freq", torch.zeros(hashtbl_size, device=device, dtype=torch.int64))
            self.register_buffer("cache_state", torch.full((hashtbl_size,), -1, device=device, dtype=torch.int32))
            self.cache_weight = nn.Parameter(torch.zeros((cache_size, self.embedding_dim), device=device, dtype=torch.float32))
            if sparse and stateful:
                shape = (cache_size, self.embedding_dim) if optimizer == OptimType.EXACT_ADAGRAD else (cache_size,)
                self.register_buffer("cache_optimizer_state", torch.zeros(shape, device=device, dtype=torch.float32))
            else:
                self.cache_optimizer_state = None
        else:
            self.register_buffer("hashtbl", torch.empty(0, device=device, dtype=torch.int64))
            self.register_buffer("cache_freq", torch.empty(0, device=device, dtype=torch.int64))
            self.register_buffer("cache_state", torch.empty(0, device=device, dtype=torch.int32))
            self.cache_optimizer_state = None
            self.cache_weight = None
        self.warmup = True

    def _key_space(self) -> List[int]:
        """the row cache keys a lookup (table k, index i) by key_base[k] + i: the running sum of the tables' prod(p), num_tables + 1
        entries (include/ttx.h "row cache over tables of different row factors")"""
        bases = self.__dict__.get("_key_bases")
        if bases is None:
            bases = [0]
            for p in self.tt_p_shapes:
                bases.append(bases[-1] + int(np.prod(np.asarray(p, dtype=object))))
            self._key_bases = bases
        return bases

    def _tables_cache(self) -> bool:
        """one row cache over the tables, however many (one table included: the parent's one-table routes take one list of row
        factors)"""
        return bool(self.use_cache)

    def cache_populate(self, write_back: float = 0.0, write_back_steps: int = 1, keep_trained: bool = False,
                       freq_shift: int = 0) -> None:
        """the cache_size most frequent keys get the cache rows, each decompressed from its own table (ttx_cache_populate_v); the
        cache is live from here on.  GPU only; no `write_back`.  `keep_trained` / `freq_shift`: as the parent's (keys cached
        before and after keep their trained rows and state; cache_freq >>= freq_shift in front of the sort)."""
        self._refresh_check(keep_trained, freq_shift)
        if not self.use_cache:
            return
        if write_back > 0.0:
            raise NotImplementedError("cache_populate(write_back > 0) is not supported by the row cache over several tables")
        populate = getattr(_ops._engine, "cache_populate_var_tables", None)
        if populate is None or not self.cache_weight.is_cuda:
            raise NotImplementedError("the row cache over tables of different row factors is populated on the GPU only")
        extra = {"reference_exact": True} if self.reference_exact_populate else {}
        old = self._refresh_begin(keep_trained, freq_shift)
        populate(self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, list(self.tt_cores), self.hashtbl, self.cache_freq,
                 self.cache_state, self.cache_weight, **extra)
        self._refresh_end(old)
        self.warmup = False
        self._drop_prefetched()

    def _table_dims(self, k: int, t: int):
        rk = self.tt_ranks if self.table_ranks is None else self.table_ranks[k]
        return rk[t], (self.tt_q_shapes if self.table_q is None else self.table_q[k])[t], rk[t + 1]

    def set_table_core(self, k: int, t: int, core: torch.Tensor) -> None:
        """core t of table k from its natural shape [p_k_t, r_t q_t r_{t+1}] (the table's own ranks and factoring), zero-padded to
        the common ones"""
        rows = self.table_rows(t)[k]
        if self.table_ranks is None and self.table_q is None:
            rows.copy_(core.reshape(rows.shape))
            return
        R0, Q, R1 = self.tt_ranks[t], self.tt_q_shapes[t], self.tt_ranks[t + 1]
        r0, q, r1 = self._table_dims(k, t)
        rows.zero_()
        rows.view(-1, R0, Q, R1)[:, :r0, :q, :r1] = core.reshape(-1, r0, q, r1)

    def table_core(self, k: int, t: int) -> torch.Tensor:
        """core t of table k in its natural shape [p_k_t, r_t q_t r_{t+1}] (a copy when the table's ranks / factoring are padded)"""
        rows = self.table_rows(t)[k]
        if self.table_ranks is None and self.table_q is None:
            return rows
        R0, Q, R1 = self.tt_ranks[t], self.tt_q_shapes[t], self.tt_ranks[t + 1]
        r0, q, r1 = self._table_dims(k, t)
        return rows.view(-1, R0, Q, R1)[:, :r0, :q, :r1].reshape(rows.shape[0], -1)

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None, warmup: bool = True,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        res = super().forward(indices, offsets, warmup, per_sample_weights)
        if self.table_q is None:
            return res
        # (after pooling, whatever the mode: sum, mean and max all pool column by column)
        return torch.gather(res, 2, self._cols.unsqueeze(1).expand(-1, res.size(1), -1))  # [tables, B, out_dim]

    def table_rows(self, t: int) -> List[torch.Tensor]:
        """views [p_k_t, slice] of core t, one per table"""
        sizes = [p[t] for p in self.tt_p_shapes]
        return list(torch.split(self.tt_cores[t].detach()[0], sizes, dim=0))

    def full_weight(self, table: Optional[int] = None) -> torch.Tensor:
        """`table` = k: table k's [E_k, D]; None: refused, as the tables have no common shape"""
        if table is None:
            raise NotImplementedError("full_weight() is per table: full_weight(k), or build a TTEmbeddingBag from table_rows()")
        k = self._table_index(table)
        return _ops._svd.tt_full(self.table_cores(k), self.table_num_embeddings[k])

    # ------------------------------------------------- canonical cores, from_pretrained
    def _no_table_q(self, what: str) -> None:
        if self.table_q is not None:
            raise NotImplementedError(f"{what} is not offered for a group of differently factored tables (table_q / pad_q): its "
                                      f"cores are stored padded to the common factoring")

    def table_cores(self, table: int = 0) -> List[torch.Tensor]:
        """table k's cores in ttx_svd's canonical form [r_k, p_k, q_k, r_{k+1}], copies -- at the table's own ranks
        (`table_ranks`), else the module's"""
        self._no_table_q("table_cores")
        k = self._table_index(table)
        rk = self.tt_ranks if self.table_ranks is None else self.table_ranks[k]
        return _ops._svd.from_module_layout([self.table_core(k, t) for t in range(self.tt_ndim)], self.tt_q_shapes, rk)

    def load_table_cores(self, cores: Sequence[torch.Tensor], table: int = 0) -> None:
        """write table k's cores from the canonical form, shapes checked.  Their ranks may be smaller than the module's (than
        `table_ranks[k]`, where given): the factor goes into the leading block of the table's slices, the rest is zero -- and
        stays zero under the fused optimizers, as the padding of `table_ranks` does."""
        self._no_table_q("load_table_cores")
        k = self._table_index(table)
        rk = self.tt_ranks if self.table_ranks is None else self.table_ranks[k]
        got = self._check_loadable(cores, self.tt_p_shapes[k], self.tt_q_shapes, rk, exact=False)
        with torch.no_grad():
            for t, c in enumerate(cores):
                rows = self.table_rows(t)[k]
                rows.zero_()
                rows.view(-1, self.tt_ranks[t], self.tt_q_shapes[t], self.tt_ranks[t + 1])[:, :got[t], :, :got[t + 1]] = \
                    c.permute(1, 0, 2, 3).to(rows)

    @classmethod
    def _construct(cls, num_embeddings, embedding_dim: int, tt_ranks, tt_p_shapes, tt_q_shapes, kw: dict):
        return cls(num_embeddings, embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, **kw)

    @classmethod
    def from_pretrained(cls, embeddings, tt_ranks: Optional[Sequence[int]] = None,
                        tt_p_shapes: Optional[Sequence[Optional[List[int]]]] = None, tt_q_shapes: Optional[List[int]] = None, *,
                        rel_error: Optional[float] = None, max_rank: Optional[int] = None, rank_multiple: int = 1,
                        **module_kwargs):
        """the parent's from_pretrained for tables of different cardinality: `embeddings` is a list with [E_k, D] per table,
        `tt_p_shapes` one list per table (or None: the constructor's default).  With `rel_error` every table is truncated at
        its own ranks and zero-padded to the per-position maximum, at which the module is built."""
        for name in ("table_q", "table_ranks"):
            if module_kwargs.get(name) is not None:
                raise NotImplementedError(f"from_pretrained does not take {name}: every table is factored at the module's "
                                          f"tt_q_shapes, and smaller ranks are zero-padded")
        _ops._check_module_kwargs(cls, module_kwargs)
        if isinstance(embeddings, torch.Tensor):
            raise ValueError("embeddings: a list with one table [E_k, D] each")
        tables = cls._pretrained_tables(embeddings, stacked=False)
        D = int(tables[0].size(1))
        nd = cls._pretrained_dims(tt_ranks, tt_p_shapes[0] if tt_p_shapes is not None and tt_p_shapes[0] is not None else None,
                                  tt_q_shapes)
        if tt_p_shapes is not None and len(tt_p_shapes) != len(tables):
            raise ValueError(f"tt_p_shapes: one list per table ({len(tables)}), got {len(tt_p_shapes)}")
        ps = [[int(x) for x in tt_p_shapes[k]] if tt_p_shapes is not None and tt_p_shapes[k] is not None
              else suggested_tt_shapes(int(w.size(0)), nd) for k, w in enumerate(tables)]
        q = [int(x) for x in tt_q_shapes] if tt_q_shapes is not None \
            else suggested_tt_shapes(D, nd, allow_round_up=not module_kwargs.get("enforce_embedding_dim", False))
        res = [_ops._svd.tt_svd(w, p, q, tt_ranks, rel_error=rel_error, max_rank=max_rank, rank_multiple=rank_multiple)
               for w, p in zip(tables, ps)]
        return cls._from_factors(res, [int(w.size(0)) for w in tables], D, ps, q, module_kwargs)

    def truncate_ranks(self, *a, **kw):
        raise NotImplementedError("truncate_ranks is offered on the one-table and the uniform batched modules: round the tables "
                                  "with ttx_svd.tt_round(table_cores(k), ..) and load them into a new module")


PAD_SENTINEL = -1  # what a table's padding slots become in a group's merged batch: no row of any table


class _MergeFunction(torch.autograd.Function):
    """`bags_merge` with per_sample_weights that require a gradient: the merged weights are the tables' weights laid end to end
    (ones where a table has none), so the backward hands every table its slice of the merged gradient."""

    @staticmethod
    def forward(ctx, indices, offsets, include_last_offset, padding, *weights):
        idx, off, w = _ops._engine.bags_merge(indices, offsets, include_last_offset, list(weights), padding, PAD_SENTINEL)
        ctx.mark_non_differentiable(idx, off)
        ctx.sizes = [int(i.numel()) for i in indices]
        ctx.shapes = [None if x is None else x.shape for x in weights]
        return idx, off, w

    @staticmethod
    def backward(ctx, _d_idx, _d_off, d_w):
        parts = d_w.split(ctx.sizes)
        return (None, None, None, None) + tuple(None if s is None else p.reshape(s) for s, p in zip(ctx.shapes, parts))


def _lookup_node(fn):
    """the autograd node that runs a group's backward kernels: `fn` itself, or the first node behind the view / reshape nodes
    the module put on top of it (a node with more than one differentiable input, or none behind it, ends the walk)"""
    seen = 0
    while fn is not None and seen < 8:
        name = type(fn).__name__
        if not any(v in name for v in ("View", "Reshape", "Slice", "Gather", "Expand", "Alias", "Unsqueeze", "Squeeze", "Permute", "Transpose", "Clone", "Contiguous")):
            return fn
        nxt = [f for f, _ in fn.next_functions if f is not None]
        if len(nxt) != 1:
            return fn
        fn, seen = nxt[0], seen + 1
    return fn


def _adam_node(fn, depth: int = 4):
    """under OptimType.EXACT_ADAM the node that enqueues a group's LAST backward kernels is not the lookup node but the
    `_AdamStepFunction` node the cores passed through, a few edges below it (behind the view / pad nodes of the q0 > 4 routes):
    that node, or None"""
    todo = [(fn, 0)]
    while todo:
        f, d = todo.pop()
        if f is None:
            continue
        if "_AdamStepFunction" in type(f).__name__:
            return f
        if d < depth:
            todo += [(g, d + 1) for g, _ in f.next_functions]
    return None


class MixedTTEmbeddingBag(nn.Module):
    """TT embedding bags for tables of different cardinality -- and, table by table, different TT ranks and different
    factorings q of the (common) embedding dimension.

    Tables that can share a launch set share one module: `self.groups[k]` is the module of group k,
    `self.group_tables[k]` its table ids.
      fused=False: a group = tables of equal (p, q, ranks), a `TableBatchedTTEmbeddingBag`;
      fused=True : a group = tables of equal factoring q whatever their row factors p AND their ranks, a `VarTableTTEmbeddingBag`:
                   ONE launch set per q -- tables of smaller ranks are stored zero-padded to the group's largest (exact: the padding
                   stays zero under the fused optimizers; costs the multiply-adds on the zeros: done by default when that is at most
                   twice the tables' own work, `pad_ranks=True / False` forces it / keeps one group per (q, ranks)).  Tables that differ in q produce
                   output rows of different layouts: separate launch sets, or -- `pad_q` (round 4; same default rule and switch) -- ONE
                   set over the entry-by-entry largest factoring, every table's cores zero-padded to it and its own values gathered
                   out of the padded rows (`VarTableTTEmbeddingBag(table_q=)`).
    `streams=True` gives every group a HIP stream of its own: eagerly the step is host-bound and nothing is gained, but
    captured into a hipGraph (ttx_graph.GraphedRound) the groups become parallel branches and their kernels -- each too
    small to fill the chip at DLRM batch sizes -- run side by side (scripts/bench_mixed.py).
    `tt_ranks` / `tt_q_shapes`: one list for all tables, or one list per table.
    `mode`, `padding_idx` (trailing keywords): nn.EmbeddingBag's pooling modes and padded batches as on the uniform modules
    (DESIGN.md 4.9 - 4.11).  `padding_idx` is None, one int, or one entry (int or None) per table, each normalised against its own
    table's cardinality.
    `dense_below` / `dense` (trailing keywords): table k stays UNCOMPRESSED when `dense[k]` is true or, without
    `dense`, when num_embeddings[k] < dense_below.  Those tables form `self.dense_groups` / `self.dense_group_tables` (one
    `DenseTableBatchedEmbeddingBag` per 64 of them: plain rows, one lookup launch, one update per touched row); `self.groups` /
    `self.group_tables` keep holding the TT groups only, so the cache fan-outs and the `cache_size` split see TT tables only.  The
    defaults select no table: same groups, same state_dict() keys, same routes.
    `use_cache=True` (with fused=True): every fused group gets ONE LFU row cache over its tables
    (`VarTableTTEmbeddingBag(use_cache=True)`).  A positive `cache_size` / `hashtbl_size` is the total over the groups, split in
    proportion to their summed cardinalities (rounded down, at least 1 each); 0 gives every group its default.  `cache_populate()`,
    `reset_cache()` and `update_cache(indices, offsets)` (per-table lists) fan out to the groups.  A group that would need
    `table_q` is refused: `pad_q=False` avoids it.
    forward(indices, offsets[, per_sample_weights]) takes one tensor per table (nn.EmbeddingBag call form,
    `include_last_offset` as given to the constructor; or, per table, 2-D `indices[k]` [B, L_k] with `offsets[k] = None`) and
    returns one [B, D] tensor per table.  On GPU tensors a group's table-major batch is ONE launch (`ttx_bags_merge`)."""

    def __init__(self, num_embeddings: Sequence[int], embedding_dim: int, tt_ranks,
                 tt_p_shapes: Optional[Sequence[Optional[List[int]]]] = None, tt_q_shapes=None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 device: Optional[torch.device] = None, include_last_offset: bool = False,
                 streams: bool = False, fused: bool = False, pad_ranks: Optional[bool] = None,
                 pad_q: Optional[bool] = None, mode: str = "sum", padding_idx=None, use_cache: bool = False,
                 cache_size: int = 0, hashtbl_size: int = 0, deterministic_cache_update: Optional[bool] = None,
                 dense_below: int = 0, dense: Optional[Sequence[bool]] = None, betas: Tuple[float, float] = (0.9, 0.999),
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False) -> None:
        super().__init__()
        if use_cache and sparse and optimizer == OptimType.EXACT_ADAM:
            raise NotImplementedError("OptimType.EXACT_ADAM does not support use_cache=True (the cache rows have no Adam state)")
        # (betas, weight_decay, decoupled_weight_decay: handed to every group; read under OptimType.EXACT_ADAM only -- one fused
        #  Adam / AdamW step per group and backward)
        adam_kw = dict(betas=betas, weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay)
        if use_cache and not fused:
            raise NotImplementedError("use_cache=True needs fused=True: the row cache is one per fused group "
                                      "(VarTableTTEmbeddingBag(use_cache=True))")
        self.use_cache = bool(use_cache)
        self.num_embeddings = [int(e) for e in num_embeddings]
        n = len(self.num_embeddings)
        if mode not in POOLING_MODES:
            raise ValueError(f"mode must be one of {POOLING_MODES}, got {mode!r}")
        self.mode = mode
        # the tables that stay uncompressed (dense_below / dense) leave the TT grouping below: tt_ids = the others
        self.dense_tables = dense_table_flags(self.num_embeddings, dense_below, dense)
        tt_ids = [k for k in range(n) if not self.dense_tables[k]]
        # padding_idx: None, one int for all tables, or one entry (an int or None) per table -- each normalised by torch's rule
        # against its OWN table's cardinality (-1 is every table's last row)
        if isinstance(padding_idx, (list, tuple)):
            if len(padding_idx) != n:
                raise ValueError(f"padding_idx: one value, or one entry per table ({n}), got {len(padding_idx)} entries")
            pads = list(padding_idx)
        else:
            pads = [padding_idx] * n
        self.padding_idx = [_normalise_padding_idx(v, e) for v, e in zip(pads, self.num_embeddings)]
        self.embedding_dim = int(embedding_dim)
        self.include_last_offset = bool(include_last_offset)
        self._streams = None
        per_table = lambda v: v is not None and len(v) > 0 and isinstance(v[0], (list, tuple))  # noqa: E731
        ranks = [[int(x) for x in r] for r in tt_ranks] if per_table(tt_ranks) else [[int(x) for x in tt_ranks]] * n
        assert len(ranks) == n, "tt_ranks: one list, or one list per table"
        if per_table(tt_q_shapes):
            qs = [[int(x) for x in q] for q in tt_q_shapes]
        else:
            qs = [None if tt_q_shapes is None else [int(x) for x in tt_q_shapes]] * n
        assert len(qs) == n, "tt_q_shapes: one list, or one list per table"
        shapes: List[Tuple[int, ...]] = []
        for k, e in enumerate(self.num_embeddings):
            nd = len(ranks[k]) + 1
            given = tt_p_shapes[k] if tt_p_shapes is not None else None
            shapes.append(tuple(int(x) for x in given) if given is not None else tuple(suggested_tt_shapes(e, nd)))
        if fused:  # (every table's factoring, spelled out: the grouping below compares them)
            qs = [q if q is not None else suggested_tt_shapes(self.embedding_dim, len(ranks[k]) + 1, allow_round_up=not enforce_embedding_dim)
                  for k, q in enumerate(qs)]

        def madds(rk, q):
            return sum(rk[i] * q[i] * rk[i + 1] for i in range(len(q)))

        # tables of different FACTORINGS in one launch set (cores zero-padded to the entry-by-entry largest factoring,
        # `VarTableTTEmbeddingBag(table_q=)`, ranks padded with them): decided per group of tables with the same number of cores
        # (round 4 advisor: one global flag q- and rank-padded EVERY group as soon as one passed the test -- possibly onto a
        # factoring outside the specialised templates).  padq_nd = the core counts whose tables share one padded set.
        padq_nd = set()
        if pad_q is None and fused:
            # auto: when the padding costs at most twice the tables' own multiply-adds
            by_nd: Dict[int, List[int]] = {}
            for k in tt_ids:
                by_nd.setdefault(len(ranks[k]), []).append(k)
            for tabs in by_nd.values():
                if len({tuple(qs[k]) for k in tabs}) < 2 or pad_ranks is False and len({tuple(ranks[k]) for k in tabs}) > 1:
                    continue
                nd1 = len(ranks[tabs[0]])
                qmax = [max(qs[k][i] for k in tabs) for i in range(nd1 + 1)]
                rmax = [max(ranks[k][i] for k in tabs) for i in range(nd1)]
                real = sum(madds([1] + ranks[k] + [1], qs[k]) for k in tabs)
                if madds([1] + rmax + [1], qmax) * len(tabs) <= 2 * real:
                    padq_nd.add(nd1)
        elif pad_q and fused:
            padq_nd = {len(ranks[k]) for k in tt_ids}
        pad_q = bool(padq_nd)
        if pad_ranks is None and fused:
            # auto: one launch set per factoring when the zero padding costs at most twice the tables' own multiply-adds
            # (measured, scripts/bench_mixed.py: ranks 32 / 16 in one set 0.278 vs 0.297 ms/step in two; ranks 64 / 32 / 16 /
            # [13,12] in one set 0.72 vs 0.43 in four)
            pad_ranks = True
            by_q: Dict[tuple, List[int]] = {}
            for k in tt_ids:
                if len(ranks[k]) in padq_nd:  # (q-padded groups pad their ranks anyway: they do not vote on the others' rule)
                    continue
                by_q.setdefault((len(ranks[k]), None if qs[k] is None else tuple(qs[k])), []).append(k)
            for tabs in by_q.values():
                qq = qs[tabs[0]] or suggested_tt_shapes(self.embedding_dim, len(ranks[tabs[0]]) + 1, allow_round_up=not enforce_embedding_dim)
                rmax = [max(ranks[k][i] for k in tabs) for i in range(len(ranks[tabs[0]]))]
                real = sum(madds([1] + ranks[k] + [1], qq) for k in tabs)
                if madds([1] + rmax + [1], qq) * len(tabs) > 2 * real:
                    pad_ranks = False
        groups: Dict[tuple, List[int]] = {}
        for k in tt_ids:
            # fused: tables of one factoring q share a batched lookup whatever their ranks (smaller ranks are zero-padded to the
            # group's largest, VarTableTTEmbeddingBag(table_ranks=)); pad_ranks=False keeps one group per (q, ranks)
            inq = len(ranks[k]) in padq_nd  # this table's core-count group shares ONE padded factoring (ranks padded with it)
            key = ((len(ranks[k]),) if fused and (pad_ranks or inq) else (tuple(ranks[k]),)) + \
                  ((len(ranks[k]),) if inq else (None if qs[k] is None else tuple(qs[k]),)) + (() if fused else (shapes[k],))
            groups.setdefault(key, []).append(k)
        self.group_tables = list(groups.values())
        self.groups = nn.ModuleList()
        # use_cache: every fused group gets a cache of its own.  A positive cache_size / hashtbl_size is the TOTAL over the groups,
        # split in proportion to the groups' summed cardinalities (rounded down, at least 1 each); 0: every group's own default
        total_rows = sum(self.num_embeddings[k] for k in tt_ids)  # (the TT tables': a dense table has no cache)
        for tables in self.group_tables:
            k0 = tables[0]
            cache_kw = {}
            if use_cache:
                share = sum(self.num_embeddings[k] for k in tables)
                cache_kw = dict(use_cache=True, deterministic_cache_update=deterministic_cache_update,
                                cache_size=max(1, int(cache_size) * share // total_rows) if cache_size > 0 else 0,
                                hashtbl_size=max(1, int(hashtbl_size) * share // total_rows) if hashtbl_size > 0 else 0)
            if fused:  # ONE batched lookup for the group's tables, whatever their row factors (VarTableTTEmbeddingBag)
                rmax = [max(ranks[k][i] for k in tables) for i in range(len(ranks[k0]))]
                mixed_ranks = any(ranks[k] != rmax for k in tables)
                qmax = [max(qs[k][i] for k in tables) for i in range(len(qs[k0]))]
                mixed_q = any(qs[k] != qmax for k in tables)
                if use_cache and mixed_q:
                    raise NotImplementedError(f"use_cache=True: tables {tables} share one launch set over a padded factoring "
                                              f"(table_q), which the row cache does not serve -- pad_q=False keeps one group (and "
                                              f"one cache) per factoring")
                self.groups.append(VarTableTTEmbeddingBag(
                    [self.num_embeddings[k] for k in tables], self.embedding_dim, rmax, [list(shapes[k]) for k in tables],
                    qmax, optimizer, learning_rate, eps, sparse, weight_dist, enforce_embedding_dim, device, True,
                    [ranks[k] for k in tables] if mixed_ranks else None, [qs[k] for k in tables] if mixed_q else None, mode,
                    **cache_kw, **adam_kw))
            else:
                self.groups.append(TableBatchedTTEmbeddingBag(
                    len(tables), max(self.num_embeddings[k] for k in tables), self.embedding_dim, list(ranks[k0]),
                    list(shapes[k0]), qs[k0], optimizer, learning_rate, eps, sparse, False, 0, 0, weight_dist,
                    enforce_embedding_dim, device, True, mode=mode, **adam_kw))
        # A group module takes ONE padding value, its tables may each have their own: forward() rewrites every table's padding
        # slots to PAD_SENTINEL and the group compacts on that.  The sentinel is no valid row, so it is handed over here -- the
        # one place -- past the constructor's normalisation, which would read -1 as "the last row".
        for mod, tables in zip(self.groups, self.group_tables):
            if any(self.padding_idx[k] is not None for k in tables):
                mod.padding_idx = PAD_SENTINEL
        self._streams = [torch.cuda.Stream(device=self.groups[0].tt_cores[0].device) for _ in self.groups] \
            if streams and len(self.groups) > 1 else None
        # the uncompressed tables: one DenseTableBatchedEmbeddingBag per 64 of them, in the caller's order; they run on the calling
        # stream.  A table's padding reaches the kernel as PAD_SENTINEL in the merged batch, which it skips itself.
        self.dense_group_tables = dense_table_groups(self.dense_tables)
        self.dense_groups = nn.ModuleList(
            DenseTableBatchedEmbeddingBag([self.num_embeddings[k] for k in tables], self.embedding_dim, optimizer, learning_rate,
                                          eps, sparse, device, True, mode, **adam_kw) for tables in self.dense_group_tables)

    # ------------------------------------------------------------------ per-table access, from_pretrained
    def _member(self, table: int):
        """-> (the group module that holds table k, its position there, whether the group is a dense one)"""
        n = len(self.num_embeddings)
        if isinstance(table, bool) or not hasattr(table, "__index__") or not -n <= int(table) < n:
            raise IndexError(f"table {table!r}: the module has {n} tables")
        k = int(table) % n
        for mods, ids, dense in ((self.groups, self.group_tables, False),
                                 (self.__dict__["_modules"].get("dense_groups", ()), self.__dict__.get("dense_group_tables", ()), True)):
            for mod, tables in zip(mods, ids):
                if k in tables:
                    return mod, tables.index(k), dense
        raise AssertionError(f"table {k} belongs to no group")

    def table_cores(self, table: int) -> List[torch.Tensor]:
        """TT table k's cores in ttx_svd's canonical form (copies)"""
        mod, j, dense = self._member(table)
        if dense:
            raise ValueError(f"table {table} is a dense member: it has rows (full_weight), not cores")
        return mod.table_cores(j)

    def load_table_cores(self, cores: Sequence[torch.Tensor], table: int) -> None:
        """write TT table k's cores from the canonical form (in a fused group: ranks up to the group's, zero-padded)"""
        mod, j, dense = self._member(table)
        if dense:
            raise ValueError(f"table {table} is a dense member: it has rows, not cores")
        mod.load_table_cores(cores, j)

    def full_weight(self, table: int) -> torch.Tensor:
        """table k's [E_k, D]: expanded from its cores, or -- a dense member -- a copy of its rows"""
        mod, j, dense = self._member(table)
        if dense:
            return mod.table_weight(j).clone()
        return mod.full_weight(j)[:self.num_embeddings[int(table) % len(self.num_embeddings)]]

    @classmethod
    def from_pretrained(cls, embeddings, tt_ranks=None, tt_p_shapes: Optional[Sequence[Optional[List[int]]]] = None,
                        tt_q_shapes=None, *, rel_error: Optional[float] = None, max_rank: Optional[int] = None,
                        rank_multiple: int = 1, **module_kwargs):
        """nn.EmbeddingBag.from_pretrained's counterpart: `embeddings` is a list with [E_k, D] per table; the TT
        members are the TT-SVD of their tables (ttx_svd.tt_svd), the dense members (`dense_below=` / `dense=`) copies of their
        rows.  `tt_ranks`: one list or one per table, as in the constructor; `rel_error` (with `max_rank` / `rank_multiple`)
        instead: every table gets the ranks its own truncation chose, three cores unless the shapes given say otherwise.
        `module_kwargs` are the constructor's.  `module.compression[k]` = (ranks, bound, norm), None for a dense member."""
        _ops._check_module_kwargs(cls, module_kwargs)
        if isinstance(embeddings, torch.Tensor):
            raise ValueError("embeddings: a list with one table [E_k, D] each")
        tables = TableBatchedTTEmbeddingBag._pretrained_tables(embeddings, stacked=False)
        n, D = len(tables), int(tables[0].size(1))
        Es = [int(w.size(0)) for w in tables]
        if (tt_ranks is None) == (rel_error is None):
            raise ValueError("exactly one of tt_ranks and rel_error must be given")
        dense = dense_table_flags(Es, module_kwargs.get("dense_below", 0), module_kwargs.get("dense"))
        per_table = lambda v: v is not None and len(v) > 0 and isinstance(v[0], (list, tuple))  # noqa: E731
        if tt_ranks is not None:
            ranks = [list(r) for r in tt_ranks] if per_table(tt_ranks) else [list(tt_ranks)] * n
            nds = [len(r) + 1 for r in ranks]
        else:
            shapes = list(tt_p_shapes or []) + (list(tt_q_shapes) if per_table(tt_q_shapes) else [tt_q_shapes])
            given = [v for v in shapes if v is not None]
            ranks, nds = [None] * n, [len(given[0]) if given else 3] * n
        if len(ranks) != n or (tt_p_shapes is not None and len(tt_p_shapes) != n):
            raise ValueError(f"tt_ranks / tt_p_shapes: one entry per table ({n})")
        qs = [list(v) for v in tt_q_shapes] if per_table(tt_q_shapes) else [None if tt_q_shapes is None else list(tt_q_shapes)] * n
        res: List[Optional[_ops._svd.TTFactors]] = [None] * n
        for k, w in enumerate(tables):
            if dense[k]:
                continue
            p = tt_p_shapes[k] if tt_p_shapes is not None and tt_p_shapes[k] is not None else suggested_tt_shapes(Es[k], nds[k])
            q = qs[k] if qs[k] is not None else suggested_tt_shapes(
                D, nds[k], allow_round_up=not module_kwargs.get("enforce_embedding_dim", False))
            res[k] = _ops._svd.tt_svd(w, p, q, ranks[k], rel_error=rel_error, max_rank=max_rank, rank_multiple=rank_multiple)
        if tt_ranks is None:  # every table at the ranks its truncation chose (a dense member's entry is not read)
            some = next((r.ranks for r in res if r is not None), [1] * (nds[0] - 1))
            tt_ranks = [list(r.ranks) if r is not None else list(some) for r in res]
        kw = dict(module_kwargs)
        kw.setdefault("weight_dist", "uniform")  # (the cheapest initialiser: the cores are overwritten)
        m = cls(Es, D, tt_ranks, tt_p_shapes, tt_q_shapes, **kw)
        with torch.no_grad():
            for k, w in enumerate(tables):
                if dense[k]:
                    mod, j, _ = m._member(k)
                    mod.table_weight(j).copy_(w)
                else:
                    m.load_table_cores(res[k].cores, k)
        m.compression = [None if r is None else (list(r.ranks), r.bound, r.norm) for r in res]
        return m

    # ------------------------------------------------------------------ the groups' row caches (use_cache=True)
    def cache_populate(self, keep_trained: bool = False, freq_shift: int = 0) -> None:
        """every group's cache_populate(keep_trained=, freq_shift=): the groups' caches are live from here on"""
        for mod in self.groups:  # (refusals first: no group is populated when one of them refuses)
            mod._refresh_check(keep_trained, freq_shift)
        for mod in self.groups:
            mod.cache_populate(keep_trained=keep_trained, freq_shift=freq_shift)

    def reset_cache(self) -> None:
        for mod in self.groups:
            mod.reset_cache()

    def update_cache(self, indices: Sequence[torch.Tensor], offsets: Sequence[Optional[torch.Tensor]]) -> None:
        """count a batch -- one (indices, offsets) pair per table, the form forward() takes -- in the groups' frequency tables;
        padding slots are not counted"""
        if not self.__dict__.get("use_cache", False):
            return
        n = len(self.num_embeddings)
        assert len(indices) == n and len(offsets) == n, f"one (indices, offsets) pair per table: {n} tables"
        for mod, tables in zip(self.groups, self.group_tables):
            idx, off, _ = self._merge(tables, indices, offsets, None)
            if mod.padding_idx is not None:  # (the merged batch holds PAD_SENTINEL at the padding: torch ops drop it, as forward's
                keep = idx != mod.padding_idx  # CPU route does; the live count shapes the result -- a host synchronisation)
                before = torch.cat([torch.zeros(1, dtype=torch.int64, device=idx.device), torch.cumsum(keep, 0)])
                idx, off = idx[keep], before[off.long().clamp(0, idx.numel())]
            mod.update_cache(idx, off)

    def _merge(self, tables: List[int], indices, offsets, per_sample_weights):
        """the batch of one group, table-major: (indices, offsets with the closing entry, weights or None), every table's padding
        slots rewritten to PAD_SENTINEL.  GPU tensors: one `bags_merge` launch (two from 65 tables on); CPU tensors (the tests'
        oracle engine): `merge_bags` and torch ops."""
        idx = [indices[k] for k in tables]
        off = [offsets[k] for k in tables]
        psw = None
        d = self.__dict__  # (a module pickled before the keywords existed has neither attribute: sum, no padding)
        if per_sample_weights is not None and any(per_sample_weights[k] is not None for k in tables):
            if d.get("mode", "sum") != "sum":
                raise ValueError(f"per_sample_weights is only supported with mode='sum' (as in torch), not mode={d['mode']!r}")
            psw = [per_sample_weights[k] for k in tables]
        pads = d.get("padding_idx")
        pads = [None] * len(tables) if pads is None else [pads[k] for k in tables]
        nb = set()
        for k, i, o in zip(tables, idx, off):
            if (i.dim() == 2) != (o is None) or i.dim() not in (1, 2):
                raise ValueError(f"table {k}: 1-D indices with 1-D offsets, or 2-D indices [B, L] with offsets None (as in torch)")
            nb.add(int(i.size(0)) if o is None else int(o.numel()) - (1 if self.include_last_offset else 0))
        if len(nb) != 1:
            raise ValueError(f"every table must describe the same number of bags, got {sorted(nb)}")
        if psw is not None:
            for k, i, w in zip(tables, idx, psw):
                if w is not None and w.shape != i.shape:
                    raise ValueError(f"table {k}: per_sample_weights must have the shape of indices")
        has_pad = any(v is not None for v in pads)
        if idx[0].is_cuda:
            if psw is not None:
                psw = [None if w is None else w.float() for w in psw]
            if psw is not None and any(w is not None and w.requires_grad for w in psw):
                return _MergeFunction.apply(idx, off, self.include_last_offset, pads if has_pad else None, *psw)
            return _ops._engine.bags_merge(idx, off, self.include_last_offset, psw, pads if has_pad else None, PAD_SENTINEL)
        entries = nb.pop() + (1 if self.include_last_offset else 0)
        flat_i, flat_o = [], []
        for i, o, v in zip(idx, off, pads):
            if o is None:  # B bags of L slots
                o = torch.arange(entries, dtype=torch.int64, device=i.device) * int(i.size(1))
                i = i.reshape(-1)
            i, o = i.long(), o.long()
            flat_i.append(i if v is None else torch.where(i == v, torch.full_like(i, PAD_SENTINEL), i))
            flat_o.append(o)
        mi, mo = merge_bags(flat_i, flat_o, self.include_last_offset)
        mw = None
        if psw is not None:
            mw = torch.cat([w.reshape(-1).float() if w is not None else torch.ones(i.numel(), device=mi.device)
                            for w, i in zip(psw, flat_i)])
        return mi, mo, mw

    def forward(self, indices: Sequence[torch.Tensor], offsets: Sequence[Optional[torch.Tensor]],
                per_sample_weights: Optional[Sequence[Optional[torch.Tensor]]] = None) -> List[torch.Tensor]:
        """per table: 1-D `indices[k]` with `offsets[k]`, or 2-D `indices[k]` [B, L_k] with `offsets[k] = None` (tables may mix the
        forms); `per_sample_weights[k]` of the shape of `indices[k]`, or None"""
        n = len(self.num_embeddings)
        assert len(indices) == n and len(offsets) == n, f"one (indices, offsets) pair per table: {n} tables"
        outs: List[Optional[torch.Tensor]] = [None] * n
        cur = torch.cuda.current_stream() if self._streams else None
        for g, (mod, tables) in enumerate(zip(self.groups, self.group_tables)):
            idx, off, psw = self._merge(tables, indices, offsets, per_sample_weights)
            if self._streams:
                s = self._streams[g]
                s.wait_stream(cur)
                with torch.cuda.stream(s):
                    res = mod(idx, off, True, psw)  # [tables, B, D]
                node = _lookup_node(res.grad_fn)
                if node is not None and mod.__dict__.get("_adam") is not None:
                    node = _adam_node(node) or node  # (the Adam step is enqueued behind the lookup's backward: join after it)
                if node is not None:
                    # autograd runs this group's backward (recompute + fused optimizer) on the group's stream as well, and
                    # with a fused optimizer there is no leaf gradient whose stream the engine would join at the end: join
                    # it here, after the node has enqueued its kernels (needed for hipGraph capture -- "unjoined work" --
                    # and for whoever reads the cores on the caller's stream next).  The hook goes on the LOOKUP node, not on
                    # whatever reshapes its result (q0 > 4 returns a view: a ViewBackward hook would fire before the lookup's
                    # backward has enqueued anything -- round 3 advisor finding)
                    node.register_hook(lambda gi, go, s=s, cur=cur: cur.wait_stream(s))
                for t in (idx, off) + ((psw,) if psw is not None else ()):
                    t.record_stream(s)   # allocated on the caller's stream, read on the group's
                res.record_stream(cur)   # ... and the other way round
            else:
                res = mod(idx, off, True, psw)
            for j, k in enumerate(tables):
                outs[k] = res[j]
        for mod, tables in zip(self.__dict__["_modules"].get("dense_groups", ()), self.__dict__.get("dense_group_tables", ())):
            idx, off, psw = self._merge(tables, indices, offsets, per_sample_weights)
            res = mod(idx, off, psw)  # [tables, B, D], on the calling stream
            for j, k in enumerate(tables):
                outs[k] = res[j]
        if self._streams:
            for s in self._streams:
                cur.wait_stream(s)
        return outs  # type: ignore[return-value]
