"""Uncompressed tables behind the batched call form: `DenseTableBatchedEmbeddingBag` (not in the reference).

A TT table of 3 rows saves no memory and costs the contraction of an 11 M-row table per lookup.  This module holds such tables
as plain rows -- ONE Parameter `weight` [R, D], table k at rows [row_base[k], row_base[k + 1]) -- and looks all of them up in one
launch (include/ttx.h `ttx_dense_bags_forward`); the backward groups the batch by row with a stable sort and updates every touched
row once, without atomics (`ttx_dense_bags_backward`: fused SGD / Adagrad, or the dense gradient).  It takes the table-major batch
of `TableBatchedTTEmbeddingBag` and returns [num_tables, B, D]; `MixedTTEmbeddingBag(dense_below=)` builds it for its small tables.
GPU tensors only; no cache, no dedup, no prefetch.
"""
from typing import List, Optional, Sequence, Tuple

import torch
from torch import nn

import tt_embeddings_ops as _ops
from tt_embeddings_ops import POOLING_MODES, OptimType, _normalise_padding_idx, _SGD_LIKE

MAX_TABLES = 64  # TTX_MAX_TABLES_MIXED: tables of one module (one launch)


class DenseLookupFunction(torch.autograd.Function):
    """forward: one launch over all tables; backward: the row-sorted update (sparse: applied here, no weight gradient) or the
    dense gradient.  The gradient of per_sample_weights is returned on both routes, from the weights before the update."""

    @staticmethod
    def forward(ctx, indices, offsets, per_sample_weights, row_base, padding, mode, optimizer, learning_rate, eps, sparse,
                optimizer_state, weight):
        out, live, arg = _ops._engine.dense_bags_forward(indices, offsets, row_base, weight, mode, padding, per_sample_weights)
        ctx.save_for_backward(indices, offsets, per_sample_weights, live, arg)
        ctx.row_base, ctx.padding, ctx.mode, ctx.sparse = row_base, padding, mode, sparse
        ctx.optimizer, ctx.learning_rate, ctx.eps = optimizer, learning_rate, eps
        ctx.optimizer_state, ctx.weight = optimizer_state, weight
        return out

    @staticmethod
    def backward(ctx, d_output):
        indices, offsets, psw, live, arg = ctx.saved_tensors
        E = _ops._engine
        want_psw = psw is not None and ctx.needs_input_grad[2]
        weight = ctx.weight.detach()
        if ctx.sparse:
            optim = E.OPTIM_SGD if ctx.optimizer in _SGD_LIKE else E.OPTIM_ADAGRAD
            state = None if optim == E.OPTIM_SGD else ctx.optimizer_state
        else:
            optim, state = E.OPTIM_DENSE, None
        d_w, d_psw = E.dense_bags_backward(optim, indices, offsets, ctx.row_base, weight, d_output.contiguous(), ctx.mode,
                                           ctx.padding, psw, live, arg, ctx.learning_rate, ctx.eps, state, want_psw)
        if d_psw is not None:
            d_psw = d_psw.view(psw.shape)
        return (None, None, d_psw) + (None,) * 8 + (d_w,)


class DenseTableBatchedEmbeddingBag(nn.Module):
    """nn.EmbeddingBag over several uncompressed tables of different cardinality in one launch set.

    `num_embeddings`: the tables' cardinalities (at most 64).  `optimizer` / `learning_rate` / `eps` / `sparse`: as on the TT
    modules -- sparse=True applies the fused update in backward (SGD / EXACT_SGD: SGD; EXACT_ROWWISE_ADAGRAD: one state value
    per row; EXACT_ADAM: torch.optim.Adam's step -- AdamW's with `decoupled_weight_decay` -- on the WHOLE weight per backward, with
    `betas` / `weight_decay`, state `optimizer_state` (exp_avg) and `optimizer_state_v` (exp_avg_sq) [R, D] and `optimizer_step`,
    DESIGN.md 4.17; every other OptimType: element-wise Adagrad, as for the TT cores), sparse=False leaves `weight.grad`.  `mode`:
    "sum" / "mean" / "max"; `padding_idx`: None, one value, or one entry per table (torch's rule against the table's own
    cardinality); negative indices in the batch are padding too (the merged batches' sentinel).
    forward(indices, offsets=None, per_sample_weights=None): the table-major batch -- 1-D indices with offsets
    (num_tables * B + 1 entries with `include_last_offset`, else num_tables * B), or 2-D [num_tables * B, L] -- -> [num_tables, B, D].
    """

    def __init__(self, num_embeddings: Sequence[int], embedding_dim: int, optimizer: OptimType = OptimType.SGD,
                 learning_rate: float = 0.1, eps: float = 1.0e-10, sparse: bool = True, device: Optional[torch.device] = None,
                 include_last_offset: bool = True, mode: str = "sum", padding_idx=None,
                 betas: Tuple[float, float] = (0.9, 0.999), weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False) -> None:
        super().__init__()
        Es = [int(e) for e in num_embeddings]
        if not 1 <= len(Es) <= MAX_TABLES or any(e <= 0 for e in Es):
            raise ValueError(f"num_embeddings: 1 to {MAX_TABLES} positive cardinalities, got {len(Es)} tables")
        if mode not in POOLING_MODES:
            raise ValueError(f"mode must be one of {POOLING_MODES}, got {mode!r}")
        if int(embedding_dim) <= 0:
            raise ValueError(f"embedding_dim must be positive, got {embedding_dim}")
        if isinstance(padding_idx, (list, tuple)):
            if len(padding_idx) != len(Es):
                raise ValueError(f"padding_idx: one value, or one entry per table ({len(Es)}), got {len(padding_idx)} entries")
            pads = list(padding_idx)
        else:
            pads = [padding_idx] * len(Es)
        self.padding_idx = [_normalise_padding_idx(v, e) for v, e in zip(pads, Es)]
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("DenseTableBatchedEmbeddingBag needs a GPU")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        self.table_num_embeddings, self.num_tables, self.embedding_dim = Es, len(Es), int(embedding_dim)
        self.mode, self.include_last_offset = mode, bool(include_last_offset)
        self.optimizer, self.learning_rate, self.eps, self.sparse = optimizer, float(learning_rate), float(eps), bool(sparse)
        self.row_base = [0]
        for e in Es:
            self.row_base.append(self.row_base[-1] + e)
        R, D = self.row_base[-1], self.embedding_dim
        self.weight = nn.Parameter(torch.empty((R, D), device=device, dtype=torch.float32))
        self._adam = None
        if self.sparse and optimizer == OptimType.EXACT_ADAM:
            self._adam = _ops._check_adam_args(betas, weight_decay) + (bool(decoupled_weight_decay),)
        if optimizer in _SGD_LIKE or (optimizer == OptimType.EXACT_ADAM and not self.sparse):
            shape = (0,)
        elif optimizer == OptimType.EXACT_ROWWISE_ADAGRAD:
            shape = (R,)
        else:
            shape = (R, D)
        self.register_buffer("optimizer_state", torch.zeros(shape, device=device, dtype=torch.float32))
        if self._adam is not None:  # (exp_avg_sq and the steps taken; optimizer_state is exp_avg)
            self.register_buffer("optimizer_state_v", torch.zeros(shape, device=device, dtype=torch.float32))
            self.register_buffer("optimizer_step", torch.zeros(1, dtype=torch.int64, device=device))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        """every table as DLRM initialises it: U(-1/sqrt(E_k), 1/sqrt(E_k))"""
        with torch.no_grad():
            for k, e in enumerate(self.table_num_embeddings):
                bound = 1.0 / float(e) ** 0.5
                self.table_weight(k).uniform_(-bound, bound)
            self.optimizer_state.zero_()
            if self.__dict__.get("_adam") is not None:
                self.optimizer_state_v.zero_()
                self.optimizer_step.zero_()

    @classmethod
    def from_pretrained(cls, embeddings: Sequence[torch.Tensor], **module_kwargs) -> "DenseTableBatchedEmbeddingBag":
        """the module whose table k holds the rows of `embeddings[k]` [E_k, D] (copied); `module_kwargs` are the constructor's.
        Beside the TT modules' from_pretrained; there is no `freeze`."""
        _ops._check_module_kwargs(cls, module_kwargs)
        tables = list(embeddings) if not isinstance(embeddings, torch.Tensor) else None
        if not tables or any(not isinstance(w, torch.Tensor) or w.dim() != 2 or not w.is_floating_point() for w in tables):
            raise ValueError("embeddings: a list of 2-D floating-point tables [E_k, D]")
        if len({int(w.size(1)) for w in tables}) != 1:
            raise ValueError("embeddings: every table needs the same embedding dimension")
        m = cls([int(w.size(0)) for w in tables], int(tables[0].size(1)), **module_kwargs)
        with torch.no_grad():
            for k, w in enumerate(tables):
                m.table_weight(k).copy_(w)
        return m

    def table_weight(self, k: int) -> torch.Tensor:
        """table k's rows [E_k, D], a view of `weight` (`table_weight(k).copy_(bag.weight)` imports an nn.EmbeddingBag)"""
        return self.weight.detach()[self.row_base[k]:self.row_base[k + 1]]

    def table_state(self, k: int) -> torch.Tensor:
        """table k's rows of `optimizer_state` (a view; empty under SGD)"""
        if self.optimizer_state.numel() == 0:
            return self.optimizer_state
        return self.optimizer_state[self.row_base[k]:self.row_base[k + 1]]

    def set_learning_rate(self, lr: float) -> None:
        self.learning_rate = float(lr)

    def _adam_step_from(self, grads) -> None:
        _ops._adam_step([self.weight.detach()], grads, [self.optimizer_state], [self.optimizer_state_v], self.optimizer_step,
                        self.learning_rate, self.eps, self._adam)

    def _offsets_2d(self, nb: int, L: int, device) -> torch.Tensor:
        cached = self.__dict__.get("_off2d")
        if cached is None or cached[0] != (nb, L, device):
            cached = ((nb, L, device), torch.arange(nb + 1, dtype=torch.int64, device=device) * L)
            self.__dict__["_off2d"] = cached
        return cached[1]

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not indices.is_cuda:
            raise RuntimeError("DenseTableBatchedEmbeddingBag: tensors must live on a GPU (there is no CPU route)")
        if indices.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"indices must be int64 or int32, got {indices.dtype}")
        if (indices.dim() == 2) != (offsets is None) or indices.dim() not in (1, 2):
            raise ValueError("1-D indices with 1-D offsets, or 2-D indices [num_tables * B, L] with offsets None (as in torch)")
        if per_sample_weights is not None:
            if self.mode != "sum":
                raise ValueError(f"per_sample_weights is only supported with mode='sum' (as in torch), not mode={self.mode!r}")
            if per_sample_weights.shape != indices.shape:
                raise ValueError("per_sample_weights must have the shape of indices")
            per_sample_weights = per_sample_weights.float()
        if offsets is None:
            nb, L = int(indices.size(0)), int(indices.size(1))
            offsets = self._offsets_2d(nb, L, indices.device)
        else:
            offsets = offsets.long()
            if not self.include_last_offset:
                offsets = torch.cat([offsets, torch.full((1,), indices.numel(), dtype=torch.int64, device=offsets.device)])
            nb = int(offsets.numel()) - 1
        if nb < 0 or nb % self.num_tables:
            raise ValueError(f"the batch must describe num_tables * B bags ({self.num_tables} tables), got {nb}")
        flat = indices.reshape(-1).long()
        pads = self.padding_idx if any(v is not None for v in self.padding_idx) else None
        weight, sparse = self.weight, self.sparse
        if self.__dict__.get("_adam") is not None:
            # EXACT_ADAM: the lookup runs as for sparse=False and its weight gradient ends in one Adam step (tt_embeddings_ops
            # `_AdamStepFunction`); an empty batch takes none
            (weight,), sparse = _ops._AdamStepFunction.apply(self, flat.numel() > 0, weight), False
        out = DenseLookupFunction.apply(flat, offsets, per_sample_weights, self.row_base, pads, self.mode, self.optimizer,
                                        self.learning_rate, self.eps, sparse, self.optimizer_state, weight)
        return out.view(self.num_tables, nb // self.num_tables, self.embedding_dim)

    def extra_repr(self) -> str:
        return (f"tables={self.num_tables}, rows={self.row_base[-1]}, dim={self.embedding_dim}, mode={self.mode}, "
                f"optimizer={self.optimizer.name}, sparse={self.sparse}")


def dense_table_flags(num_embeddings: Sequence[int], dense_below: int = 0,
                      dense: Optional[Sequence[bool]] = None) -> List[bool]:
    """which tables of a mixed module stay uncompressed: `dense[k]` when `dense` is given, else num_embeddings[k] < dense_below
    (the defaults select none).  Pure: needs no GPU."""
    n = len(num_embeddings)
    if dense is not None:
        if len(dense) != n:
            raise ValueError(f"dense: one flag per table ({n}), got {len(dense)}")
        return [bool(v) for v in dense]
    if int(dense_below) < 0:
        raise ValueError(f"dense_below must not be negative, got {dense_below}")
    return [int(e) < int(dense_below) for e in num_embeddings]


def dense_table_groups(flags: Sequence[bool]) -> List[List[int]]:
    """the dense tables' ids in the caller's order, MAX_TABLES per group (one module, one launch set each)"""
    ids = [k for k, f in enumerate(flags) if f]
    return [ids[i:i + MAX_TABLES] for i in range(0, len(ids), MAX_TABLES)]
