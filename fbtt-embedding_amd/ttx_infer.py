"""TTInferenceBag: a frozen, forward-only copy of a trained TT module that serves its lookups from bf16 cores (not in the
reference; include/ttx.h "bf16 inference forward").

    served = TTInferenceBag.from_module(trained)      # TTEmbeddingBag, TableBatchedTTEmbeddingBag or TTEmbedding
    out = served(indices, offsets)                    # the source's call forms, float32 out, nothing requires grad

The cores are rounded ONCE to bf16 (round to nearest even, `tensor.to(torch.bfloat16)`).  Where the bf16 kernel takes the geometry
(`route == "bf16"`: three cores, ranks <= 64) they are kept in its packed layout as buffers and a call is the lookup prologue,
`tt_rows_bf16`, `bag_sum_pool` (and `bag_mean_scale` for mode="mean").  Everywhere else (`route == "fp32"`: two or four cores,
larger ranks) the module keeps the SAME rounded weights as float32 in the ordinary layout, inside a parameter-free twin of the
source, and calls the existing fp32 forward: the call always works, with the same rounding of the weights.  On CPU tensors the
bf16 route computes the same chain product with torch ops from the packed cores (what the tests run without a GPU).

`from_module(trained, wide=True)` opts in to the column-blocked kernel for the three-core geometries the narrow
one refuses -- ranks up to 128, any q1 <= 64: `route == "bf16w"`, the same packed buffers, `tt_rows_bf16w` in place of
`tt_rows_bf16`.  Every other geometry keeps the route it has without the flag.

`from_module(trained, mfma_tail=True)` opts in to the kernel that runs BOTH products on the bf16 MFMA for the
geometries the two above refuse for their last factor -- q2 up to 32, the default factorings of every width from 640 up:
`route == "bf16m"`, core 2 packed transposed, `tt_rows_bf16m`.  It rounds x_0 once to bf16: within the same bound, not bit-equal
to the fp32 route.

`from_module(trained, four_cores=True)` opts in to the four-core kernel for tables of FOUR cores with ranks
<= 64 and q2 q3 <= 32: `route == "bf16q"`, four packed buffers, `tt_rows_bf16q` -- all three products on the bf16 MFMA in chain
order (core_0 core_1) (core_2 core_3), both factors rounded once to bf16 in LDS: within its own bound (include/ttx.h), not
bit-equal to the fp32 route.  Routes are tried in the order "bf16", "bf16w" (with `wide`), "bf16m" (with `mfma_tail`), "bf16q"
(with `four_cores`), "fp32".

`from_module(trained, fused_bags=True)` opts in to the POOLED one-launch kernel for a TTEmbeddingBag or
TableBatchedTTEmbeddingBag whose geometry it takes (three cores, ranks <= 64, q0 q1 <= 64, q2 <= 32): `route == "bf16b"`, tried
FIRST when asked for, the packed buffers of `pack_cores_bf16m`.  A call is the call-form normalisation and ONE `tt_bags_bf16`
launch -- no prologue, no plan, no rows, no pooling launch: a wave walks a bag's lookups and sums them in its MFMA accumulators.
Only this route serves what every source module serves and the others refuse: a source with `padding_idx` (the value is kept; such
slots are skipped and not counted for the mean) and `forward(indices, offsets, per_sample_weights=w)` (float32, the numel of
indices, mode "sum" only).  Within its own bound (include/ttx.h), not bit-equal to the other routes; a TTEmbedding source or a
geometry outside the domain keeps the route it gets without the flag; a hot table with the flag is refused.

`from_module(trained, hot_indices=rows)` (one 1-D int64 tensor, or one per table) keeps those rows EXPANDED beside the cores
(DESIGN.md 4.23): computed once through the module's own route, rounded to bf16, as the buffers `hot_keys` [K] (sorted, key =
table * num_embeddings + index) and `hot_rows` [K, D]; `hot_rows_count` is K.  A call then probes the table, pools the hits from
it, compacts the misses on the device and contracts only those (`hot_probe_pool`, `bags_compact`, the prologue and rows kernel on
the live count, `bag_sum_pool_add`): a bag is its hits in slot order, then its misses in slot order -- within the bound, not
bit-equal to the module without the table.  `from_module(cached, hot_from_cache=True)` freezes a module whose row cache is LIVE:
the hot set is what it holds cached, the hot rows are its trained `cache_weight` rows.  Routes "bf16", "bf16w", "bf16m" and
"bf16q"; the "fp32" route refuses a hot table (its twin hands out no rows).  Without either argument nothing changes.

Limits: the bf16 kernels take three cores, or four with ranks <= 64 and q2 q3 <= 32 (two cores, four beyond that: "fp32"); no
fp16 / fp8 weights; rows and output stay float32; padding_idx and per_sample_weights on route "bf16b" only, where one bag is
one work-group (a very long bag is not split); no mode="max"; a live row
cache only as the hot table above (which is fixed at freeze time), not the mixed-cardinality or sharded module classes (the C
entry points do take p_tables geometries); nothing trains."""
from typing import List, Optional, Sequence

import torch
from torch import nn

import tt_embeddings as _engine
import tt_embeddings_ops as _ops


def _pad_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def packed_shapes(q: Sequence[int], ranks: Sequence[int], mfma_tail: bool = False):
    """(per-slice shape of each packed core, the valid extents inside it) of a three-core geometry; ranks = [1, r1, r2, 1];
    mfma_tail: core 2 in the transposed layout of the MFMA-tail kernel, [Q2P = q2 up to 16][K2p = r2 up to 32].  Four factors
    in q (ranks = [1, r1, r2, r3, 1]): the layout of the four-core kernel, core 2 [r2 q2][K3p], core 3 transposed [16][K3p]"""
    r1, r2 = int(ranks[1]), int(ranks[2])
    K1p, N1 = _pad_up(r1, 32), int(q[1]) * r2
    if len(q) == 4:
        r3, K3p = int(ranks[3]), _pad_up(int(ranks[3]), 32)
        return ([(int(q[0]), K1p), (_pad_up(N1, 16), K1p), (r2 * int(q[2]), K3p), (16, K3p)],
                [(int(q[0]), r1), (N1, r1), (r2 * int(q[2]), r3), (int(q[3]), r3)])
    q0, q1, q2 = (int(x) for x in q)
    last = ((_pad_up(q2, 16), _pad_up(r2, 32)), (q2, r2)) if mfma_tail else ((r2, 4 if q2 <= 4 else 8), (r2, q2))
    return ([(q0, K1p), (_pad_up(N1, 16), K1p), last[0]], [(q0, r1), (N1, r1), last[1]])


def pack_cores_torch(cores: Sequence[torch.Tensor], q: Sequence[int], ranks: Sequence[int],
                     mfma_tail: bool = False) -> List[torch.Tensor]:
    """the packed bf16 layout of include/ttx.h with torch ops (any device): what ttx_tt_pack_bf16 (mfma_tail:
    ttx_tt_pack_bf16m; four cores: ttx_tt_pack_bf16q) writes, bit for bit"""
    full, valid = packed_shapes(q, ranks, mfma_tail)
    r1, r2 = int(ranks[1]), int(ranks[2])
    four = len(q) == 4
    out = []
    for t, c in enumerate(cores):
        c = c.detach().reshape(-1, c.size(-1))  # [slices, r q r']
        S = c.size(0)
        if t == 1:  # [r1][q1 r2] -> column-major: K contiguous per output column
            c = c.view(S, r1, -1).transpose(1, 2)
        if t == 2 and mfma_tail and not four:  # [r2][q2] -> [q2][r2]: K contiguous per output column
            c = c.view(S, r2, -1).transpose(1, 2)
        if t == 3:  # [r3][q3] -> [q3][r3]: K contiguous per output column
            c = c.view(S, int(ranks[3]), -1).transpose(1, 2)
        c = c.reshape(S, *valid[t]).to(torch.bfloat16)
        pk = torch.zeros((S,) + full[t], dtype=torch.bfloat16, device=c.device)
        pk[:, :valid[t][0], :valid[t][1]] = c
        out.append(pk.reshape(-1))
    return out


def unpack_cores_torch(packed: Sequence[torch.Tensor], q: Sequence[int], ranks: Sequence[int],
                       mfma_tail: bool = False) -> List[torch.Tensor]:
    """-> float32 cores [slices, r q r'] in the ordinary layout, holding exactly the bf16 values"""
    full, valid = packed_shapes(q, ranks, mfma_tail)
    out = []
    for t, pk in enumerate(packed):
        c = pk.view(-1, *full[t])[:, :valid[t][0], :valid[t][1]].float()
        if t == 1 or t == 3 or (t == 2 and mfma_tail and len(q) == 3):
            c = c.transpose(1, 2)
        out.append(c.reshape(c.size(0), -1).contiguous())
    return out


class TTInferenceBag(nn.Module):
    """see the module docstring; build with `TTInferenceBag.from_module(module)`"""

    def __init__(self) -> None:
        super().__init__()
        self.route = "bf16"

    @classmethod
    def from_module(cls, module: nn.Module, wide: bool = False, mfma_tail: bool = False, hot_indices=None,
                    hot_from_cache: bool = False, four_cores: bool = False, fused_bags: bool = False) -> "TTInferenceBag":
        if not isinstance(module, _ops.TableBatchedTTEmbeddingBag) or isinstance(module.tt_p_shapes[0], (list, tuple)) \
                or hasattr(module, "_p_flat"):
            raise TypeError("TTInferenceBag.from_module takes a TTEmbeddingBag, a TableBatchedTTEmbeddingBag or a TTEmbedding, got "
                            f"{type(module).__name__} (the mixed-cardinality and sharded classes are out of scope)")
        mode = module.__dict__.get("mode", "sum")
        if mode == "max":
            raise ValueError("TTInferenceBag: mode='max' is not supported (the inference path pools by sum or mean)")
        fused = bool(fused_bags) and not isinstance(module, _ops.TTEmbedding) and _engine.tt_bags_bf16_supported(
            module.num_tables, list(module.tt_p_shapes), list(module.tt_q_shapes), list(module.tt_ranks))
        if fused and (hot_from_cache or hot_indices is not None):
            raise ValueError("TTInferenceBag: a hot row table is not served with fused_bags=True -- the hot path is built on "
                             "compaction and rows, the pooled kernel has neither; drop one of the two")
        padding_idx = module.__dict__.get("padding_idx")
        if padding_idx is not None and not fused:
            raise ValueError("TTInferenceBag: a module with padding_idx is not supported")
        live = bool(module.use_cache and not module.warmup)
        if live and not hot_from_cache:
            raise ValueError("TTInferenceBag: the module's row cache is live -- its cached rows were trained away from the cores, "
                             "and a copy of the cores would serve stale rows; fold them back with cache_populate(write_back=...) "
                             "and reset_cache(), or freeze a fresh module")
        if hot_from_cache and not live:
            raise ValueError("TTInferenceBag: hot_from_cache=True takes a module whose row cache is live (after cache_populate())")
        if hot_from_cache and hot_indices is not None:
            raise ValueError("TTInferenceBag: give hot_indices or hot_from_cache=True, not both")
        self = cls()
        self.kind = "embedding" if isinstance(module, _ops.TTEmbedding) else \
            ("bag" if isinstance(module, _ops.TTEmbeddingBag) else "batched")
        self.num_tables, self.num_embeddings, self.embedding_dim = module.num_tables, module.num_embeddings, module.embedding_dim
        self.tt_p_shapes, self.tt_q_shapes = list(module.tt_p_shapes), list(module.tt_q_shapes)
        self.tt_ranks = list(module.tt_ranks)
        self.mode, self.include_last_offset = mode, bool(module.include_last_offset)
        cores = [c.detach() for c in module.tt_cores]
        geom = (self.num_tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks)
        self.padding_idx = padding_idx  # (None on every route but "bf16b")
        if fused:
            self.route = "bf16b"  # (opt-in, tried first: one pooled launch, weights and padding inside the walk)
        elif _engine.tt_rows_bf16_supported(*geom):
            self.route = "bf16"
        elif wide and _engine.tt_rows_bf16w_supported(*geom):
            self.route = "bf16w"  # (opt-in: the column-blocked kernel where the narrow one refuses)
        elif mfma_tail and _engine.tt_rows_bf16m_supported(*geom):
            self.route = "bf16m"  # (opt-in: both products on the MFMA, q2 up to 32)
        elif four_cores and _engine.tt_rows_bf16q_supported(*geom):
            self.route = "bf16q"  # (opt-in: four cores, all three products on the MFMA)
        else:
            self.route = "fp32"
        if self.route == "fp32" and (hot_from_cache or hot_indices is not None):
            raise ValueError("TTInferenceBag: a hot row table is not served on route 'fp32' -- the twin pools inside its own forward "
                             "and hands out no rows for a compacted batch to add to the hits' sums; it needs a geometry of the "
                             "bf16 kernels (three cores, or four with four_cores=True; wide=True / mfma_tail=True widen the domain)")
        if self.route != "fp32":
            if cores[0].is_cuda:
                pack = {"bf16": _engine.pack_cores_bf16, "bf16w": _engine.pack_cores_bf16w, "bf16m": _engine.pack_cores_bf16m,
                        "bf16q": _engine.pack_cores_bf16q, "bf16b": _engine.pack_cores_bf16m}
                packed = pack[self.route](*geom, cores)
            else:
                packed = pack_cores_torch(cores, self.tt_q_shapes, self.tt_ranks, self.route in ("bf16m", "bf16b"))
            for t, pk in enumerate(packed):
                self.register_buffer(f"packed_core{t}", pk)
        else:
            # the same rounding of the weights on the fp32 kernels: a twin of the source built by its own constructor (no
            # cache, no optimizer state) whose cores are BUFFERS holding the bf16 values as float32
            kw = module._ctor_kwargs()
            kw.update(use_cache=False, sparse=False, optimizer=_ops.OptimType.SGD, dedup=False, weight_dist="uniform")
            kw.pop("cache_size", None), kw.pop("hashtbl_size", None)
            twin = type(module)._construct([self.num_embeddings] * self.num_tables, self.embedding_dim, self.tt_ranks[1:-1],
                                           self.tt_p_shapes, self.tt_q_shapes, kw)
            del twin.tt_cores
            twin.tt_cores = _ops.BufferList("tt_cores", [c.to(torch.bfloat16).float() for c in cores])
            self.fp32 = twin
        if hot_from_cache:
            self._hot_from_cache(module)
        elif hot_indices is not None:
            self._hot_from_indices(hot_indices, cores[0].device)
        return self

    # ------------------------------------------------------------------ the hot row table
    @property
    def hot_rows_count(self) -> int:
        """K: rows served from the hot table (0: there is none, and a call is what it was without one)"""
        return int(self.hot_keys.numel()) if hasattr(self, "hot_keys") else 0

    def _set_hot(self, keys: torch.Tensor, rows: torch.Tensor) -> None:
        """keys ascending and distinct, rows [K, D] bf16 in their order; K == 0 registers nothing"""
        if keys.numel() > 0:
            self.register_buffer("hot_keys", keys.contiguous())
            self.register_buffer("hot_rows", rows.contiguous())

    def _hot_from_indices(self, hot_indices, dev: torch.device) -> None:
        per_table = [hot_indices] if isinstance(hot_indices, torch.Tensor) else list(hot_indices)
        if len(per_table) != self.num_tables:
            raise ValueError(f"hot_indices: one 1-D int64 tensor per table, got {len(per_table)} for {self.num_tables} tables")
        E, keys = self.num_embeddings, []
        for t, idx in enumerate(per_table):
            if not isinstance(idx, torch.Tensor) or idx.dim() != 1 or idx.dtype != torch.int64:
                raise ValueError(f"hot_indices[{t}] must be a 1-D int64 tensor")
            if idx.numel() > 0 and (int(idx.min()) < 0 or int(idx.max()) >= E):
                raise ValueError(f"hot_indices[{t}] holds a row outside [0, {E})")
            keys.append(torch.unique(idx.to(dev)) + t * E)  # (sorted; table-major: ascending as a whole)
        keys = torch.cat(keys)
        if keys.numel() == 0:
            return
        idx, tab = keys % E, keys // E
        rows = self._rows_hip(idx, tab) if keys.is_cuda else self._rows_torch(idx, tab)  # the frozen module's own route
        self._set_hot(keys, rows.to(torch.bfloat16))

    def _hot_from_cache(self, module: nn.Module) -> None:
        """the keys the source holds cached and their cache_weight rows, read from its cache state on the host.  The source keys by
        table * prod(tt_p_shapes) + index; a cached index beyond num_embeddings has no key here and is left to the cores."""
        state, tbl = module.cache_state.cpu(), module.hashtbl.cpu()
        slots = torch.nonzero(state >= 0).flatten()
        src, loc = tbl[slots], state[slots].long()
        stride, E = module._key_stride(), self.num_embeddings
        tab, idx = src // stride, src % stride
        keep = (src >= 0) & (idx < E) & (tab < self.num_tables)
        keys, order = torch.sort(tab[keep] * E + idx[keep], stable=True)
        loc = loc[keep][order]
        first = torch.ones_like(keys, dtype=torch.bool)
        first[1:] = keys[1:] != keys[:-1]  # (a key seated twice: the lower slot's row)
        dev = module.cache_weight.device
        rows = module.cache_weight.detach()[loc[first].to(dev)].to(torch.bfloat16)
        self._set_hot(keys[first].to(dev), rows)

    def _forward_hot(self, flat: torch.Tensor, offsets: torch.Tensor, tables: int) -> torch.Tensor:
        """-> [bags, D]: every bag's hit rows from the table, then its miss rows from the cores (sum; the mean on top)"""
        E, D, nb = self.num_embeddings, self.embedding_dim, offsets.numel() - 1
        if flat.is_cuda:
            masked, out = _engine.hot_probe_pool(flat, offsets, tables, E, self.hot_keys, self.hot_rows)
            misses, miss_off, n_live = _engine.bags_compact(masked, offsets, 0, -1)
            _, tableidx, plan = _engine.lookup_prologue(misses, miss_off, tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks,
                                                        n_dev=n_live)
            rows = self._rows_hip(misses, tableidx, plan)
            out = _engine.bag_sum_pool_add(rows, miss_off, out)
            return _engine.bag_mean_scale(out, offsets) if self.mode == "mean" else out
        lens = offsets[1:] - offsets[:-1]
        bag = torch.repeat_interleave(torch.arange(nb, dtype=torch.int64), lens)
        tab = bag // (nb // tables)
        inside = (flat >= 0) & (flat < E)
        key = torch.where(inside, tab * E + flat, torch.zeros_like(flat))
        pos = torch.searchsorted(self.hot_keys, key).clamp(max=self.hot_rows_count - 1)
        hit = inside & (self.hot_keys[pos] == key)
        out = torch.zeros((nb, D), dtype=torch.float32).index_add_(0, bag[hit], self.hot_rows[pos[hit]].float())
        out.index_add_(0, bag[~hit], self._rows_torch(flat[~hit], tab[~hit]))
        if self.mode == "mean":
            out = out / lens.clamp(min=1).to(torch.float32).unsqueeze(1)
        return out

    def _forward_fused(self, flat: torch.Tensor, offsets: torch.Tensor, weights: Optional[torch.Tensor]) -> torch.Tensor:
        """route "bf16b" -> [bags, D]: ONE launch on a GPU; on CPU tensors the same sum from _rows_torch, with padding dropped and
        weights applied by torch ops"""
        nb, D, pad = offsets.numel() - 1, self.embedding_dim, self.padding_idx
        if flat.is_cuda:
            return _engine.tt_bags_bf16(self.num_tables, D, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, flat, offsets,
                                        self._packed(), weights, pad, self.mode == "mean")
        lens = offsets[1:] - offsets[:-1]
        bag = torch.repeat_interleave(torch.arange(nb, dtype=torch.int64), lens)
        keep = flat != pad if pad is not None else torch.ones_like(flat, dtype=torch.bool)
        rows = self._rows_torch(flat[keep], bag[keep] // (nb // self.num_tables))
        if weights is not None:
            rows = rows * weights[keep].unsqueeze(1)
        out = torch.zeros((nb, D), dtype=torch.float32).index_add_(0, bag[keep], rows)
        if self.mode == "mean":
            live = torch.zeros(nb, dtype=torch.int64).index_add_(0, bag, keep.long())
            out = out / live.clamp(min=1).to(torch.float32).unsqueeze(1)
        return out

    def extra_repr(self) -> str:
        hot = f", hot_rows={self.hot_rows_count}" if self.hot_rows_count else ""
        return (f"{self.kind}, route={self.route}, num_tables={self.num_tables}, p={self.tt_p_shapes}, q={self.tt_q_shapes}, "
                f"ranks={self.tt_ranks[1:-1]}, mode={self.mode}{hot}")

    def _packed(self) -> List[torch.Tensor]:
        return [getattr(self, f"packed_core{t}") for t in range(len(self.tt_q_shapes))]

    # ------------------------------------------------------------------ rows of the bf16 routes
    def _rows_hip(self, flat: torch.Tensor, tableidx: Optional[torch.Tensor], plan=None) -> torch.Tensor:
        rows = {"bf16": _engine.tt_rows_bf16, "bf16w": _engine.tt_rows_bf16w, "bf16m": _engine.tt_rows_bf16m,
                "bf16q": _engine.tt_rows_bf16q}[self.route]
        n = 1 if tableidx is None else self.num_tables
        return rows(n, self.embedding_dim, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, flat, tableidx, self._packed(), plan)

    def _rows_torch(self, flat: torch.Tensor, tableidx: Optional[torch.Tensor]) -> torch.Tensor:
        """CPU tensors (any device, really): the chain product in float32 from the packed cores"""
        if len(self.tt_q_shapes) == 4:
            return self._rows_torch4(flat, tableidx)
        c0, c1, c2 = unpack_cores_torch(self._packed(), self.tt_q_shapes, self.tt_ranks, self.route in ("bf16m", "bf16b"))
        p, q, (r1, r2) = self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks[1:3]
        idx = flat.clamp(min=0)
        i2 = (idx % p[2]).clamp(max=p[2] - 1)
        i1 = ((idx // p[2]) % p[1])
        i0 = (idx // (p[1] * p[2])).clamp(max=p[0] - 1)
        tab = tableidx if tableidx is not None else torch.zeros_like(idx)
        a = c0[tab * p[0] + i0].view(-1, q[0], r1)
        b = c1[tab * p[1] + i1].view(-1, r1, q[1] * r2)
        c = c2[tab * p[2] + i2].view(-1, r2, q[2])
        x0 = torch.bmm(a, b).view(-1, q[0] * q[1], r2)
        return torch.bmm(x0, c).reshape(-1, self.embedding_dim)

    def _rows_torch4(self, flat: torch.Tensor, tableidx: Optional[torch.Tensor]) -> torch.Tensor:
        """four cores in chain order: (core_0 core_1) (core_2 core_3)"""
        c0, c1, c2, c3 = unpack_cores_torch(self._packed(), self.tt_q_shapes, self.tt_ranks)
        p, q, (r1, r2, r3) = self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks[1:4]
        idx = flat.clamp(min=0)
        i3 = idx % p[3]
        i2 = (idx // p[3]) % p[2]
        i1 = (idx // (p[2] * p[3])) % p[1]
        i0 = (idx // (p[1] * p[2] * p[3])).clamp(max=p[0] - 1)
        tab = tableidx if tableidx is not None else torch.zeros_like(idx)
        a = c0[tab * p[0] + i0].view(-1, q[0], r1)
        b = c1[tab * p[1] + i1].view(-1, r1, q[1] * r2)
        c = c2[tab * p[2] + i2].view(-1, r2 * q[2], r3)
        d = c3[tab * p[3] + i3].view(-1, r3, q[3])
        x0 = torch.bmm(a, b).view(-1, q[0] * q[1], r2)
        m = torch.bmm(c, d).view(-1, r2, q[2] * q[3])
        return torch.bmm(x0, m).reshape(-1, self.embedding_dim)

    def _bags(self, indices: torch.Tensor, offsets: Optional[torch.Tensor]):
        """the source's call forms -> (flat int64 indices, closed int64 offsets)"""
        if offsets is None:
            if indices.dim() != 2:
                raise ValueError("indices must be [N, L] when offsets is None (N = num_tables * B bags of L slots)")
            N, L = int(indices.size(0)), int(indices.size(1))
            offsets = torch.arange(0, N * L + 1, max(L, 1), dtype=torch.int64, device=indices.device)[:N + 1] if L > 0 \
                else torch.zeros(N + 1, dtype=torch.int64, device=indices.device)
            return indices.reshape(-1).long().contiguous(), offsets
        if indices.dim() != 1 or offsets.dim() != 1:
            raise ValueError("indices and offsets must be 1-D")
        indices, offsets = indices.long().contiguous(), offsets.long()
        if not self.include_last_offset:
            offsets = torch.cat([offsets, offsets.new_full((1,), indices.numel())])
        return indices, offsets.contiguous()

    @torch.no_grad()
    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bags: 1-D indices with offsets, or [N, L] with offsets=None -> [num_tables, B, D] ([B, D] from a TTEmbeddingBag, as
        its source returns); a TTEmbedding source: indices of any shape -> indices.shape + (D,).  float32, no grad.
        per_sample_weights (route "bf16b" only): float32, the numel of indices, mode "sum"."""
        if indices.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"indices must be int64 or int32, got {indices.dtype}")
        if per_sample_weights is not None:
            if self.route != "bf16b":
                raise ValueError("TTInferenceBag: per_sample_weights are served by from_module(..., fused_bags=True) only "
                                 f"(route 'bf16b'); this module is on route {self.route!r}")
            if self.mode != "sum":
                raise ValueError(f"per_sample_weights is only supported with mode='sum' (as in torch), not mode={self.mode!r}")
            if per_sample_weights.numel() != indices.numel():
                raise ValueError("per_sample_weights must have the shape of indices")
            if per_sample_weights.dtype != torch.float32:
                raise ValueError(f"per_sample_weights must be float32, got {per_sample_weights.dtype}")
            per_sample_weights = per_sample_weights.detach().reshape(-1).contiguous()
        D = self.embedding_dim
        if self.route == "fp32":
            out = self.fp32(indices) if self.kind == "embedding" else self.fp32(indices, offsets)
            return out.detach()
        if self.kind == "embedding":
            flat = indices.reshape(-1).long().contiguous()
            if flat.numel() == 0:
                return torch.zeros(tuple(indices.shape) + (D,), dtype=torch.float32, device=indices.device)
            if self.hot_rows_count:  # (the positions as bags of one slot)
                one = torch.arange(flat.numel() + 1, dtype=torch.int64, device=flat.device)
                return self._forward_hot(flat, one, 1).view(tuple(indices.shape) + (D,))
            if flat.is_cuda:
                rows = self._rows_hip(flat, None)
            else:
                rows = self._rows_torch(flat, None)
            return rows.view(tuple(indices.shape) + (D,))
        flat, offsets = self._bags(indices, offsets)
        nb = offsets.numel() - 1
        if nb % self.num_tables != 0:
            raise ValueError(f"offsets must describe num_tables * B bags, got {nb} bags for {self.num_tables} tables")
        B = nb // self.num_tables
        shape = (B, D) if self.kind == "bag" else (self.num_tables, B, D)
        if flat.numel() == 0:
            return torch.zeros(shape, dtype=torch.float32, device=flat.device)
        if self.hot_rows_count:
            return self._forward_hot(flat, offsets, self.num_tables).view(shape)
        if self.route == "bf16b":
            return self._forward_fused(flat, offsets, per_sample_weights).view(shape)
        if flat.is_cuda:
            _, tableidx, plan = _engine.lookup_prologue(flat, offsets, self.num_tables, self.tt_p_shapes, self.tt_q_shapes,
                                                        self.tt_ranks)
            rows = self._rows_hip(flat, tableidx, plan)
            out = _engine.bag_sum_pool(rows, offsets)
            if self.mode == "mean":
                out = _engine.bag_mean_scale(out, offsets)
            return out.view(shape)
        lens = offsets[1:] - offsets[:-1]
        bag = torch.repeat_interleave(torch.arange(nb, dtype=torch.int64), lens)
        rows = self._rows_torch(flat, bag // B)
        out = torch.zeros((nb, D), dtype=torch.float32).index_add_(0, bag, rows)
        if self.mode == "mean":
            out = out / lens.clamp(min=1).to(torch.float32).unsqueeze(1)
        return out.view(shape)
