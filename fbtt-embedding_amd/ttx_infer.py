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

Limits: no fp16 / fp8 weights; rows and output stay float32; no padding_idx, no mode="max", no per_sample_weights, no live row
cache, not the mixed-cardinality or sharded module classes (the C entry points do take p_tables geometries); nothing trains."""
from typing import List, Optional, Sequence

import torch
from torch import nn

import tt_embeddings as _engine
import tt_embeddings_ops as _ops


def _pad_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def packed_shapes(q: Sequence[int], ranks: Sequence[int]):
    """(per-slice shape of each packed core, the valid extents inside it) of a three-core geometry; ranks = [1, r1, r2, 1]"""
    q0, q1, q2 = (int(x) for x in q)
    r1, r2 = int(ranks[1]), int(ranks[2])
    K1p, N1 = _pad_up(r1, 32), q1 * r2
    return ([(q0, K1p), (_pad_up(N1, 16), K1p), (r2, 4 if q2 <= 4 else 8)], [(q0, r1), (N1, r1), (r2, q2)])


def pack_cores_torch(cores: Sequence[torch.Tensor], q: Sequence[int], ranks: Sequence[int]) -> List[torch.Tensor]:
    """the packed bf16 layout of include/ttx.h with torch ops (any device): what ttx_tt_pack_bf16 writes, bit for bit"""
    full, valid = packed_shapes(q, ranks)
    r1 = int(ranks[1])
    out = []
    for t, c in enumerate(cores):
        c = c.detach().reshape(-1, c.size(-1))  # [slices, r q r']
        S = c.size(0)
        if t == 1:  # [r1][q1 r2] -> column-major: K contiguous per output column
            c = c.view(S, r1, -1).transpose(1, 2)
        c = c.reshape(S, *valid[t]).to(torch.bfloat16)
        pk = torch.zeros((S,) + full[t], dtype=torch.bfloat16, device=c.device)
        pk[:, :valid[t][0], :valid[t][1]] = c
        out.append(pk.reshape(-1))
    return out


def unpack_cores_torch(packed: Sequence[torch.Tensor], q: Sequence[int], ranks: Sequence[int]) -> List[torch.Tensor]:
    """-> float32 cores [slices, r q r'] in the ordinary layout, holding exactly the bf16 values"""
    full, valid = packed_shapes(q, ranks)
    out = []
    for t, pk in enumerate(packed):
        c = pk.view(-1, *full[t])[:, :valid[t][0], :valid[t][1]].float()
        if t == 1:
            c = c.transpose(1, 2)
        out.append(c.reshape(c.size(0), -1).contiguous())
    return out


class TTInferenceBag(nn.Module):
    """see the module docstring; build with `TTInferenceBag.from_module(module)`"""

    def __init__(self) -> None:
        super().__init__()
        self.route = "bf16"

    @classmethod
    def from_module(cls, module: nn.Module) -> "TTInferenceBag":
        if not isinstance(module, _ops.TableBatchedTTEmbeddingBag) or isinstance(module.tt_p_shapes[0], (list, tuple)) \
                or hasattr(module, "_p_flat"):
            raise TypeError("TTInferenceBag.from_module takes a TTEmbeddingBag, a TableBatchedTTEmbeddingBag or a TTEmbedding, got "
                            f"{type(module).__name__} (the mixed-cardinality and sharded classes are out of scope)")
        mode = module.__dict__.get("mode", "sum")
        if mode == "max":
            raise ValueError("TTInferenceBag: mode='max' is not supported (the inference path pools by sum or mean)")
        if module.__dict__.get("padding_idx") is not None:
            raise ValueError("TTInferenceBag: a module with padding_idx is not supported")
        if module.use_cache and not module.warmup:
            raise ValueError("TTInferenceBag: the module's row cache is live -- its cached rows were trained away from the cores, "
                             "and a copy of the cores would serve stale rows; fold them back with cache_populate(write_back=...) "
                             "and reset_cache(), or freeze a fresh module")
        self = cls()
        self.kind = "embedding" if isinstance(module, _ops.TTEmbedding) else \
            ("bag" if isinstance(module, _ops.TTEmbeddingBag) else "batched")
        self.num_tables, self.num_embeddings, self.embedding_dim = module.num_tables, module.num_embeddings, module.embedding_dim
        self.tt_p_shapes, self.tt_q_shapes = list(module.tt_p_shapes), list(module.tt_q_shapes)
        self.tt_ranks = list(module.tt_ranks)
        self.mode, self.include_last_offset = mode, bool(module.include_last_offset)
        cores = [c.detach() for c in module.tt_cores]
        if _engine.tt_rows_bf16_supported(self.num_tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks):
            self.route = "bf16"
            if cores[0].is_cuda:
                packed = _engine.pack_cores_bf16(self.num_tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, cores)
            else:
                packed = pack_cores_torch(cores, self.tt_q_shapes, self.tt_ranks)
            for t, pk in enumerate(packed):
                self.register_buffer(f"packed_core{t}", pk)
        else:
            # the same rounding of the weights on the fp32 kernels: a twin of the source built by its own constructor (no
            # cache, no optimizer state) whose cores are BUFFERS holding the bf16 values as float32
            self.route = "fp32"
            kw = module._ctor_kwargs()
            kw.update(use_cache=False, sparse=False, optimizer=_ops.OptimType.SGD, dedup=False, weight_dist="uniform")
            kw.pop("cache_size", None), kw.pop("hashtbl_size", None)
            twin = type(module)._construct([self.num_embeddings] * self.num_tables, self.embedding_dim, self.tt_ranks[1:-1],
                                           self.tt_p_shapes, self.tt_q_shapes, kw)
            del twin.tt_cores
            twin.tt_cores = _ops.BufferList("tt_cores", [c.to(torch.bfloat16).float() for c in cores])
            self.fp32 = twin
        return self

    def extra_repr(self) -> str:
        return (f"{self.kind}, route={self.route}, num_tables={self.num_tables}, p={self.tt_p_shapes}, q={self.tt_q_shapes}, "
                f"ranks={self.tt_ranks[1:-1]}, mode={self.mode}")

    def _packed(self) -> List[torch.Tensor]:
        return [self.packed_core0, self.packed_core1, self.packed_core2]

    # ------------------------------------------------------------------ rows of the bf16 route
    def _rows_torch(self, flat: torch.Tensor, tableidx: Optional[torch.Tensor]) -> torch.Tensor:
        """CPU tensors (any device, really): the chain product in float32 from the packed cores"""
        c0, c1, c2 = unpack_cores_torch(self._packed(), self.tt_q_shapes, self.tt_ranks)
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
    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bags: 1-D indices with offsets, or [N, L] with offsets=None -> [num_tables, B, D] ([B, D] from a TTEmbeddingBag, as
        its source returns); a TTEmbedding source: indices of any shape -> indices.shape + (D,).  float32, no grad."""
        if indices.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"indices must be int64 or int32, got {indices.dtype}")
        D = self.embedding_dim
        if self.route == "fp32":
            out = self.fp32(indices) if self.kind == "embedding" else self.fp32(indices, offsets)
            return out.detach()
        if self.kind == "embedding":
            flat = indices.reshape(-1).long().contiguous()
            if flat.numel() == 0:
                return torch.zeros(tuple(indices.shape) + (D,), dtype=torch.float32, device=indices.device)
            if flat.is_cuda:
                rows = _engine.tt_rows_bf16(1, D, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, flat, None, self._packed())
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
        if flat.is_cuda:
            _, tableidx, plan = _engine.lookup_prologue(flat, offsets, self.num_tables, self.tt_p_shapes, self.tt_q_shapes,
                                                        self.tt_ranks)
            rows = _engine.tt_rows_bf16(self.num_tables, D, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, flat, tableidx,
                                        self._packed(), plan)
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
