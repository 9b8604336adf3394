"""`tt_embeddings_ops` -- the TTEmbeddingBag module surface on top of libttx.

Same public names, constructor keywords, forward() call form, autograd contract
and state_dict keys as the reference's tt_embeddings_ops.py, so a model that
uses `TTEmbeddingBag` / `TableBatchedTTEmbeddingBag` in place of
`nn.EmbeddingBag(mode="sum", include_last_offset=True)` switches by import
path only.  All compute goes through the module `tt_embeddings` of this package
(ctypes -> C ABI -> hand-written HIP for gfx950); nothing here computes on the
CPU.

Reference map (file:line in /root/reference/tt_embeddings_ops.py):
  OptimType :18-33 | BufferList :36-77 | tt_matrix_to_full :80-127 |
  TTLookupFunction :130-356 | suggested_tt_shapes :359-418 |
  TableBatchedTTEmbeddingBag :421-886 | TTEmbeddingBag :889-934

Deliberate differences (each is a superset or a fix):
  * optional trailing ctor keyword `device` (default: current GPU);
  * D % 4 != 0 is supported; the README's toy example (E=10, D=3) runs;
  * `cache_optimizer_state` lives on the module's device (the reference leaves
    it on the CPU, :582-585); `reset_cache()` works (:795 has a typo);
    `get_params()` does not grow the ParameterList on every call (:882-886);
  * fused optimizers update every looked-up slice (the reference's apply-kernel
    grid skips rows);
  * nn.EmbeddingBag call forms: ctor keyword `include_last_offset` (default True =
    the reference's form), int32 indices / offsets, forward keyword
    `per_sample_weights`;
  * nn.EmbeddingBag pooling modes: ctor keyword `mode` ("sum" = the reference's, "mean", "max";
    TTMeanPoolFunction / TTMaxLookupFunction below);
  * nn.EmbeddingBag's padded batches: ctor keyword `padding_idx` and the 2-D fixed-length input `indices[N, L]` with
    `offsets=None`; the padding is dropped on the device (`bags_compact`) in front of the lookup;
  * nn.Embedding's unpooled lookup: the module `TTEmbedding` (one row per index of an index tensor of any shape, `padding_idx`;
    TTRowsLookupFunction below), on the ctypes route;
  * one row cache over the tables of a table-batched bag: `TableBatchedTTEmbeddingBag(num_tables > 1, use_cache=True)` (the
    reference asserts one table, :456) keys one hash table / cache_weight by table * prod(tt_p_shapes) + index
    (TTTablesCachedLookupFunction below), on the ctypes route -- and, for tables of different row factors
    (ttx_mixed.VarTableTTEmbeddingBag(use_cache=True)), by key_base[table] + index through the same node;
  * nn.EmbeddingBag.from_pretrained's counterpart: the classmethod `from_pretrained` (TT-SVD of dense tables, ttx_svd.py),
    `truncate_ranks` (TT rounding into a new module), `table_cores` / `load_table_cores` (one table's cores in a
    layout-independent form) and `full_weight(table)` for any number of tables;
  * when ttx_torch.so is built the lookup runs as a C++ autograd node (same C ABI
    calls as TTLookupFunction below, which stays the reference-shaped route); with a
    live cache that node keeps the partition's split point on the device instead of
    reading it back every step, and in dense mode it always returns a (possibly zero)
    gradient for cache_weight.
"""
import itertools
import logging
import math
import os
from operator import is_ as _is
from weakref import ref as _weakref
import random
from enum import Enum, unique
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

import tt_embeddings as _engine  # the 11-function native-module surface
import ttx_svd as _svd  # TT-SVD / rounding behind from_pretrained and truncate_ranks (pure torch)

_native = None  # ttx_torch (csrc/ttx_torch.cpp), False once an import attempt failed


def _native_node():
    """The C++ autograd node of the lookup, when it was built (__graft_entry__.build()) and the engine is
    the HIP shim (tests swap `_engine` for the oracle-backed stand-in on CPU).  It is an optional,
    faster route through the SAME C ABI -- TTLookupFunction below stays the reference-shaped path."""
    global _native
    if getattr(_engine, "__name__", "") != "tt_embeddings" or os.environ.get("TTX_NO_NATIVE_NODE"):
        return None
    if _engine._lib is not None and _engine._lib is _engine._hooks:
        return None  # a test / ablation knob is set: calls go to libttx_hooks.so, which the C++ node is not linked against
    if _native is None:
        try:
            import ttx_torch as _m

            _native = _m
        except ImportError:
            _native = False
    return _native or None


# ---- `out.backward(grad)` of a lookup's own output, past autograd's engine: OPT-IN --------------------------------------------------
# The reference benchmark's loop is `tt_emb(indices, offsets).backward(grad)` (tt_embeddings_benchmark.py:94-108); with a fused
# optimizer the graph under that output is the lookup's one node, which returns no gradient to anybody, and autograd's engine
# spends ~40 us of host time per step (graph task, hand-over to its device thread and back) on calling it -- more than the step's
# kernels take.  `enable_direct_backward()` (or TTX_DIRECT_BACKWARD=1 in the environment at import) wraps `torch.Tensor.backward`
# ONCE; importing this module leaves torch untouched (round 6: a drop-in that rewrites a core torch method on import is not
# reviewable; in a DLRM the lookup's output is never the tensor `.backward()` is called on, so this serves benchmark-shaped loops
# only).  While enabled, the module registers the tensors it returns on the C++ node's route (`_direct_register`), and the wrapper
# calls the node on the calling thread for exactly those tensors (csrc/ttx_torch.cpp NodeRef::backward_of) when the call is the
# plain one: a gradient and nothing else (no retain_graph / create_graph / inputs=), a plain torch.Tensor (no subclass), no
# TorchFunctionMode active, no hooks or retain_grad() on the tensor, and the tensor's grad_fn STILL the lookup's node (an in-place
# op on the output rebases it: the engine's job); NodeRef::backward itself declines on hooks on the node, anomaly mode, another
# current stream than the forward's, a gradient that is part of a graph or has the wrong shape.  Everything declined, every other
# tensor and every other USE of the output (operand of further ops, torch.autograd.backward / grad) is the original
# Tensor.backward.  The registry is a side table keyed by id() with a weak reference per entry: nothing is stored ON the tensor
# (torch.save / pickle of an output see no foreign attribute), an entry goes when its tensor goes.
# `disable_direct_backward()` puts the original method back.
_DIRECT_BACKWARD = False
_direct: Dict[int, tuple] = {}  # id(output tensor) -> (weak reference to it, NodeRef)
_tensor_backward = None  # torch.Tensor.backward as it was when enable_direct_backward() wrapped it


class _KeyRef(_weakref):
    __slots__ = ("key",)


def _direct_drop(wr) -> None:
    _direct.pop(wr.key, None)


def _direct_register(out: torch.Tensor, ref) -> None:
    wr = _KeyRef(out, _direct_drop)
    wr.key = id(out)
    _direct[wr.key] = (wr, ref)


def _backward(self, gradient=None, retain_graph=None, create_graph=False, inputs=None):
    if _direct:
        e = _direct.get(id(self))
        # (a gradient of another type or shape goes to the engine for the engine's own error)
        if (e is not None and e[0]() is self and _DIRECT_BACKWARD and type(self) is torch.Tensor and type(gradient) is torch.Tensor
                and not retain_graph and not create_graph and inputs is None and gradient.shape == self.shape
                and not self._backward_hooks and not self.retains_grad and not torch._C._len_torch_function_stack()
                and e[1].backward_of(self, gradient)):
            return None
    return _tensor_backward(self, gradient, retain_graph, create_graph, inputs)


def enable_direct_backward() -> None:
    """Opt in: `out.backward(grad)` of a fused-optimizer lookup's own output calls the lookup's node on the calling thread
    (see above).  Wraps torch.Tensor.backward once, process-wide, until disable_direct_backward()."""
    global _DIRECT_BACKWARD, _tensor_backward
    if torch.Tensor.backward is not _backward:
        _tensor_backward = torch.Tensor.backward
        _backward.__doc__ = _tensor_backward.__doc__
        torch.Tensor.backward = _backward
    _DIRECT_BACKWARD = True


def disable_direct_backward() -> None:
    """Undo enable_direct_backward(): torch.Tensor.backward is the method it was; registered outputs are forgotten."""
    global _DIRECT_BACKWARD
    _DIRECT_BACKWARD = False
    _direct.clear()
    if torch.Tensor.backward is _backward:
        torch.Tensor.backward = _tensor_backward


def direct_backward_enabled() -> bool:
    return _DIRECT_BACKWARD and torch.Tensor.backward is _backward


if os.environ.get("TTX_DIRECT_BACKWARD", "0") not in ("", "0"):
    enable_direct_backward()


@unique
class OptimType(Enum):
    SGD = "sgd"
    EXACT_SGD = "exact_sgd"
    LAMB = "lamb"
    ADAM = "adam"
    EXACT_ADAGRAD = "exact_adagrad"
    EXACT_ROWWISE_ADAGRAD = "exact_row_wise_adagrad"
    LARS_SGD = "lars_sgd"
    PARTIAL_ROWWISE_ADAM = "partial_row_wise_adam"
    PARTIAL_ROWWISE_LAMB = "partial_row_wise_lamb"
    EXACT_ADAM = "exact_adam"  # (not in the reference: torch.optim.Adam / AdamW on the cores, fused -- DESIGN.md 4.17)

    def __str__(self) -> str:
        return self.value


_SGD_LIKE = (OptimType.SGD, OptimType.EXACT_SGD)  # everything else -> Adagrad kernel (:221,:248)
# dedup="auto" policy (measured crossover): the map + pre-sum + gather pooling cost about a quarter of the plain
# step at 327k lookups, so sharing pays below ~0.7 distinct pairs per lookup; 0.6 leaves a margin
_DEDUP_AUTO_MIN_NNZ = int(os.environ.get("TTX_DEDUP_AUTO_MIN_NNZ", 65536))
_DEDUP_AUTO_MAX_DISTINCT = 0.6
_DEDUP_AUTO_PERIOD = 256


def _split0_factor(q: Sequence[int], ranks: Sequence[int]) -> int:
    """k > 1: a T = 3 table with q0 = k q0' (2 <= q0' <= 4, k <= 4), q1, q2 <= 8 and ranks <= 128 is contracted as k part
    lookups per index in the table [k p0, p1, p2] x [q0', q1, q2] -- core 0 [p0, q0, r1] IS [k p0, q0', r1] -- which the
    shape-specialised kernels take (include/ttx.h "core-0 row split"; the reference's default factoring of D = 512 is
    [8, 8, 8]).  0: no split."""
    if len(q) != 3 or q[0] <= 4 or q[1] > 16 or q[2] > 32 or max(ranks) > 128 or os.environ.get("TTX_NO_SPLIT0"):
        return 0
    if q[2] > 16 and max(ranks) > 32:  # (q2 up to 32 -- a prime last factor 17 .. 31, round 5 -- at ranks <= 32)
        return 0
    if q[2] > 8 and max(ranks) > 64:  # (q2 up to 16 -- D = 640 / 768 / 1024 -- has templates at ranks <= 64 only)
        return 0
    if q[1] > 8 and max(ranks) > 64:  # (q1 up to 16 -- D = 720 / 800 / 864 / 880 / 960 / 1008, round 5 -- at ranks <= 64)
        return 0
    for k in (2, 3, 4):
        if q[0] % k == 0 and 2 <= q[0] // k <= 4:
            return k
    return 0


def _pad0_target(q: Sequence[int], ranks: Sequence[int]) -> int:
    """Q > q0: a T = 3 table whose q0 > 4 has no exact part split (5, 7, 10, 11, 13, 14, 15) is contracted with core 0 stored
    zero-padded to Q = the next multiple of 4 slots -- [p0, Q, r1] IS [Q/4 p0, 4, r1], the part lookups of `_split0_factor` --
    and the output rows' first D values kept (q0 is the outermost factor of an output row: the real values are a prefix of
    the padded row).  Exact: the padded slots of core 0 are zero and stay zero (their gradient has the zero output gradient
    as a factor); costs the multiply-adds on them.  The reference's default factorings of D = 320 / 448 are [5, 8, 8] /
    [7, 8, 8].  0: no padding."""
    if len(q) != 3 or q[0] <= 4 or q[0] > 16 or _split0_factor(q, ranks):
        return 0
    Q = -(-q[0] // 4) * 4
    return Q if _split0_factor([Q] + list(q[1:]), ranks) else 0


class BufferList(nn.Module):
    """An indexable list of registered buffers named `<name><i>` (state_dict
    keys `optimizer_state.optimizer_state0`, ...)."""

    def __init__(self, name: str, buffers: Optional[Sequence[torch.Tensor]] = None) -> None:
        super().__init__()
        self._name = name
        self._count = 0
        for b in buffers or ():
            self.append(b)

    def append(self, buffer: torch.Tensor) -> "BufferList":
        self.register_buffer(f"{self._name}{self._count}", buffer)
        self._count += 1
        return self

    def extend(self, buffers: Sequence[torch.Tensor]) -> "BufferList":
        for b in buffers:
            self.append(b)
        return self

    def __len__(self) -> int:
        return self._count

    def __getitem__(self, index: int) -> torch.Tensor:
        if not -self._count <= index < self._count:
            raise IndexError(index)
        return getattr(self, f"{self._name}{index % self._count}")

    def __iter__(self) -> Iterator[torch.Tensor]:
        return (self[i] for i in range(self._count))


def tt_matrix_to_full(tt_p_shapes: List[int], tt_q_shapes: List[int], tt_ranks: List[int],
                      tt_cores: Sequence[torch.Tensor], tt_permute: Optional[List[int]] = None) -> torch.Tensor:
    """Expand TT cores to the dense [prod(p), prod(q)] matrix (test oracle /
    `full_weight`).  With tt_permute=[1,0,2,3] the cores are in the module's
    storage layout [1, p, r*q*r']; otherwise they are [r, p, q, r'] tensors."""
    T = len(tt_p_shapes)
    ranks = list(tt_ranks)
    if len(ranks) == T - 1:
        ranks = [1] + ranks + [1]
    mats = []
    for t, core in enumerate(tt_cores):
        shape = [ranks[t], tt_p_shapes[t], tt_q_shapes[t], ranks[t + 1]]
        if tt_permute is not None:
            stored = [shape[a] for a in tt_permute]
            core = core.reshape(stored).permute(*tt_permute)
        else:
            core = torch.squeeze(core)
        if list(core.shape) != shape:
            raise ValueError(f"core {t}: expected {shape}, got {list(core.shape)}")
        mats.append(core.contiguous())
    acc = mats[0]
    for t in range(1, T):
        acc = acc.reshape(-1, ranks[t]) @ mats[t].reshape(ranks[t], -1)
    inter = [d for pq in zip(tt_p_shapes, tt_q_shapes) for d in pq]
    acc = acc.reshape(inter)
    order = list(range(0, 2 * T, 2)) + list(range(1, 2 * T, 2))
    n_rows = int(np.prod(np.asarray(tt_p_shapes, dtype=np.int64)))
    n_cols = int(np.prod(np.asarray(tt_q_shapes, dtype=np.int64)))
    full = acc.permute(order).contiguous().reshape(n_rows, n_cols)
    return full if full.dtype == torch.float64 else full.float()  # (float64 cores: a float64 table, for the tests' references)


# --------------------------------------------------------------------------- #
# what the lookup nodes below share: the optimizer dispatch of the cores' and the cache rows' update, and the gradient tuple
# --------------------------------------------------------------------------- #

def _optim_code(sparse: bool, optimizer: OptimType) -> Tuple[bool, int]:
    """-> (use_state, optim): whether the optimizer keeps a state (Adagrad), and the C++ node's code of the update
    (0 fused SGD, 1 fused Adagrad, 2 dense gradients)."""
    use_state = sparse and optimizer not in _SGD_LIKE
    return use_state, 2 if not sparse else (1 if use_state else 0)


def _num_tables(tt_p_shapes, tt_cores) -> int:
    if len(tt_p_shapes) > 0 and isinstance(tt_p_shapes[0], (list, tuple)):
        return len(tt_p_shapes)  # tables of different row factors: cores are [1, sum p, slice]
    return tt_cores[0].size(0)


def _stash(ctx, D: int, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer: OptimType, learning_rate: float, eps: float, sparse: bool,
           optimizer_state, tt_cores) -> None:
    """what the update helpers below read off a node's ctx"""
    ctx.geometry = (tt_p_shapes, tt_q_shapes, tt_ranks)
    ctx.D = D
    ctx.optimizer, ctx.learning_rate, ctx.eps, ctx.sparse = optimizer, learning_rate, eps, sparse
    ctx.tt_cores, ctx.optimizer_state = tt_cores, optimizer_state


def _update_cores_rows(ctx, D: int, nnz: int, indices, tableidx, d_rows) -> Optional[List[torch.Tensor]]:
    """The cores' update from one gradient row per lookup, on ctx.plan: fused SGD / Adagrad in place (-> None), or the dense
    core gradients."""
    p, q, ranks = ctx.geometry
    if not ctx.sparse:
        optim, lr, eps, state = _engine.OPTIM_DENSE, 0.0, 0.0, None
    elif ctx.optimizer in _SGD_LIKE:
        optim, lr, eps, state = _engine.OPTIM_SGD, ctx.learning_rate, 0.0, None
    else:
        optim, lr, eps, state = _engine.OPTIM_ADAGRAD, ctx.learning_rate, ctx.eps, list(ctx.optimizer_state)
    return _engine.tt_backward_rows(optim, D, lr, eps, p, q, ranks, nnz, indices, tableidx, d_rows, list(ctx.tt_cores), state,
                                    ctx.plan)


def _update_cores_bags(ctx, L, nnz: int, indices, rowidx, tableidx, d_output) -> Optional[List[torch.Tensor]]:
    """The cores' update from the bags' gradient (the reference's three entry points), on ctx.plan when there is one (the
    tests' CPU engine takes no such keyword): fused SGD / Adagrad in place (-> None), or the dense core gradients."""
    p, q, ranks = ctx.geometry
    extra = {"plan": ctx.plan} if ctx.plan is not None else {}
    cores = list(ctx.tt_cores)
    if not ctx.sparse:
        return _engine.tt_dense_backward(1000, ctx.D, p, q, ranks, L, nnz, indices, rowidx, tableidx, d_output, cores, **extra)
    if ctx.optimizer in _SGD_LIKE:
        _engine.tt_sgd_backward(1000, ctx.D, ctx.learning_rate, p, q, ranks, L, nnz, indices, rowidx, tableidx, d_output, cores,
                                **extra)
    else:
        _engine.tt_adagrad_backward(1000, ctx.D, ctx.learning_rate, ctx.eps, p, q, ranks, L, nnz, indices, rowidx, tableidx,
                                    d_output, ctx.optimizer_state, cores, **extra)
    return None


def _update_cache_rows(ctx, det: Optional[bool], batch: int, nnz: int, d_output, cache_locations, rowidx, cache_optimizer_state,
                       cache_weight, skip_dev: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """The cache rows' update: SGD / row-wise Adagrad in place (-> None), or the dense gradient of cache_weight.  `det` is the
    module's deterministic_cache_update; None ("auto") looks at the BATCH (`batch` = misses + hits), as the C++ node does
    (csrc/ttx_torch.cpp kSortedAutoNnz: its split point stays on the device): all routes switch at the same batch size.  The
    engine's own default would look at the cached part alone.  The two keywords are passed only when set (None is their
    default; the tests' CPU engine takes neither)."""
    adagrad, _ = _optim_code(ctx.sparse, ctx.optimizer)
    auto = getattr(_engine, "_use_sorted", None)
    if det is None and auto is not None:
        det = auto(None, batch, adagrad=adagrad)
    kw = {} if det is None else {"deterministic": det}
    if skip_dev is not None:
        kw["skip_dev"] = skip_dev
    if not ctx.sparse:
        return _engine.cache_backward_dense(nnz, d_output, cache_locations, rowidx, ctx.learning_rate, cache_weight, **kw)
    if adagrad:
        _engine.cache_backward_rowwise_adagrad_approx(nnz, d_output, cache_locations, rowidx, ctx.learning_rate, ctx.eps,
                                                      cache_optimizer_state, cache_weight, **kw)
    else:
        _engine.cache_backward_sgd(nnz, d_output, cache_locations, rowidx, ctx.learning_rate, cache_weight, **kw)
    return None


def _grad_tuple(node, n_cores: int, core_grads=None, d_cache_weight: Optional[torch.Tensor] = None) -> tuple:
    """backward's result for `node`: None for each of its N_ARGS non-core arguments -- but for `d_cache_weight`, where there is
    one, at CACHE_WEIGHT_ARG --, then one entry per core (None under a fused optimizer)."""
    head: List[Optional[torch.Tensor]] = [None] * node.N_ARGS
    if d_cache_weight is not None:
        head[node.CACHE_WEIGHT_ARG] = d_cache_weight
    return tuple(head + (list(core_grads) if core_grads is not None else [None] * n_cores))


# --------------------------------------------------------------------------- #
# OptimType.EXACT_ADAM (not in the reference): torch.optim.Adam / AdamW on the cores, applied in backward
# --------------------------------------------------------------------------- #
# TT cores have no sparsity a lazy optimizer could use, so the semantics are torch.optim.Adam's: every element of every core
# steps at every backward.  The module runs every one of its lookup routes exactly as it runs them for sparse=False (dense core
# gradients: `_route_args`), with the cores passed through `_AdamStepFunction` first: forward hands the cores on as they are,
# backward receives all core gradients in ONE call, applies the step (`_engine.adam_apply`: two launches for all cores) and
# returns no gradient -- the cores' .grad stays None, as under the other fused optimizers.  No lookup node, kernel or route
# choice knows about it.

def _check_adam_args(betas, weight_decay: float) -> Tuple[float, float, float]:
    b1, b2 = (float(b) for b in betas)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas must lie in [0, 1), got {tuple(betas)!r}")
    if not float(weight_decay) >= 0.0:
        raise ValueError(f"weight_decay must not be negative, got {weight_decay!r}")
    return b1, b2, float(weight_decay)


def _adam_apply_torch(weights, grads, exp_avg, exp_avg_sq, step, lr, betas, eps, weight_decay=0.0, decoupled=False) -> None:
    """`_engine.adam_apply`'s formula with torch ops: what the step runs on CPU tensors (the tests' oracle engine has no
    adam_apply).  Reads the step back: not for GPU tensors."""
    b1, b2 = betas
    t = int(step.item()) + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    with torch.no_grad():
        for w, g, m, v in zip(weights, grads, exp_avg, exp_avg_sq):
            g = g.reshape(w.shape)
            if weight_decay != 0.0:
                if decoupled:
                    w.mul_(1.0 - lr * weight_decay)
                else:
                    g = g.add(w, alpha=weight_decay)
            m.mul_(b1).add_(g, alpha=1.0 - b1)
            v.mul_(b2).addcmul_(g, g, value=1.0 - b2)
            w.addcdiv_(m, v.sqrt().mul_(1.0 / math.sqrt(bc2)).add_(eps), value=-lr / bc1)
        step.add_(1)


def _adam_step(weights, grads, exp_avg, exp_avg_sq, step, lr, eps, adam) -> None:
    """one Adam step on `weights` (detached Parameters) in place; `adam` = (beta1, beta2, weight_decay, decoupled)"""
    grads = [g if g.is_contiguous() else g.contiguous() for g in grads]
    fn = getattr(_engine, "adam_apply", None)
    if fn is None or not weights[0].is_cuda:
        fn = _adam_apply_torch
    fn(weights, grads, exp_avg, exp_avg_sq, step, float(lr), (adam[0], adam[1]), float(eps), adam[2], adam[3])


class _AdamStepFunction(torch.autograd.Function):
    """The cores (or a dense group's weight) on their way into a lookup under OptimType.EXACT_ADAM.  forward: the tensors as they
    are.  backward: ONE Adam step of `module` from all their gradients (`module._adam_step_from`), no gradient handed on.
    `live` False (an empty batch): no step."""

    @staticmethod
    def forward(ctx, module, live: bool, *tensors: torch.Tensor):
        ctx.module, ctx.live = module, live
        return tuple(t.view_as(t) for t in tensors)

    @staticmethod
    def backward(ctx, *grads):
        if ctx.live:
            ctx.module._adam_step_from(grads)
        return (None, None) + (None,) * len(grads)


class TTLookupFunction(torch.autograd.Function):
    """Autograd node of one (table-batched) TT lookup.  Argument order and the
    gradient tuple (19 x None, `d_cache_weight` in slot 17 for dense mode, then
    one entry per core) follow the reference (:133-155, :280-356)."""

    N_ARGS, CACHE_WEIGHT_ARG = 19, 17  # (of forward's arguments after ctx, in front of the cores)

    @staticmethod
    def forward(ctx, B: int, D: int, tt_p_shapes: List[int], tt_q_shapes: List[int], tt_ranks: List[int],
                L: torch.Tensor, nnz_tt: int, nnz_cached: int, indices: torch.Tensor, rowidx: torch.Tensor,
                tableidx: torch.Tensor, optimizer: OptimType, learning_rate: float, eps: float, sparse: bool,
                cache_locations: Optional[torch.Tensor], cache_optimizer_state: Optional[torch.Tensor],
                cache_weight: Optional[torch.Tensor], optimizer_state: List[torch.Tensor],
                *tt_cores: torch.Tensor) -> torch.Tensor:
        _stash(ctx, D, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer, learning_rate, eps, sparse, optimizer_state, tt_cores)
        ctx.nnz_tt, ctx.nnz_cached = nnz_tt, nnz_cached
        ctx.has_cache = cache_weight is not None
        ctx.save_for_backward(L, indices, rowidx, tableidx, cache_locations, cache_optimizer_state, cache_weight)
        num_tables = _num_tables(tt_p_shapes, tt_cores)
        # one lookup plan serves forward and backward of this batch
        mk = getattr(_engine, "make_plan", None)
        ctx.plan = getattr(rowidx, "_ttx_plan", None)  # built by the module's lookup prologue
        ctx.det = getattr(rowidx, "_ttx_det", None)    # the module's deterministic_cache_update (None: the engine's default)
        if ctx.plan is None and mk is not None:
            ctx.plan = mk(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, nnz_tt, indices, tableidx, rowidx)
        extra = {"plan": ctx.plan} if ctx.plan is not None else {}
        output = _engine.tt_forward(1000, num_tables, B, D, tt_p_shapes, tt_q_shapes, tt_ranks, L, nnz_tt, indices,
                                    rowidx, tableidx, list(tt_cores), **extra)
        if nnz_cached > 0:
            _engine.cache_forward(B, nnz_cached, cache_locations[nnz_tt:], rowidx[nnz_tt:], cache_weight, output)
        return output

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        L, indices, rowidx, tableidx, cache_locations, cache_optimizer_state, cache_weight = ctx.saved_tensors
        n_tt, n_c = ctx.nnz_tt, ctx.nnz_cached
        d_output = d_output.contiguous()
        grads = _update_cores_bags(ctx, L, n_tt, indices, rowidx, tableidx, d_output)
        d_cache_weight = None
        if n_c > 0:
            d_cache_weight = _update_cache_rows(ctx, ctx.det, n_tt + n_c, n_c, d_output, cache_locations[n_tt:], rowidx[n_tt:],
                                                cache_optimizer_state, cache_weight)
        return _grad_tuple(TTLookupFunction, len(ctx.tt_cores), grads, d_cache_weight)


# --------------------------------------------------------------------------- #
# pooling modes other than sum (nn.EmbeddingBag mode="mean" / "max"; include/ttx.h "pooling modes")
# --------------------------------------------------------------------------- #

POOLING_MODES = ("sum", "mean", "max")


def _normalise_padding_idx(padding_idx, num_embeddings: int) -> Optional[int]:
    """torch.nn.EmbeddingBag's rule: None, or an int in [-num_embeddings, num_embeddings), negative values counted from the
    end; stored normalised.  Anything else is a ValueError."""
    if padding_idx is None:
        return None
    if isinstance(padding_idx, bool) or not isinstance(padding_idx, (int, np.integer)):
        raise ValueError(f"padding_idx must be None or an int, got {padding_idx!r}")
    padding_idx = int(padding_idx)
    if not -num_embeddings <= padding_idx < num_embeddings:
        raise ValueError(f"padding_idx must be within [-{num_embeddings}, {num_embeddings}), got {padding_idx}")
    return padding_idx + num_embeddings if padding_idx < 0 else padding_idx


class TTMeanPoolFunction(torch.autograd.Function):
    """mode="mean" around whatever the sum lookup returned: forward divides each bag's sum by its length, backward hands each
    lookup the same share of its bag's gradient (the sum route's backward / fused optimizer then runs on the scaled gradient).
    Empty bags stay zero."""

    @staticmethod
    def forward(ctx, summed: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(offsets)
        return _engine.bag_mean_scale(summed.contiguous(), offsets)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        (offsets,) = ctx.saved_tensors
        return _engine.bag_mean_scale(d_output.contiguous(), offsets), None


class TTMaxLookupFunction(torch.autograd.Function):
    """mode="max": the lookup's rows [nnz, D] (contraction without pooling), then the column-wise max per bag with the winning
    lookup recorded per column (the first one on a tie, as PyTorch).  Backward: the bag gradient goes, column by column, to the
    winning lookup's row only (a gradient row per lookup), and the ordinary backward / fused optimizer runs on those rows.  The
    lookup plan is built without bag rows, so that forward and backward share it (four cores: the merged last cores too)."""

    N_ARGS = 12

    @staticmethod
    def forward(ctx, B: int, D: int, tt_p_shapes: List[int], tt_q_shapes: List[int], tt_ranks: List[int],
                indices: torch.Tensor, offsets: torch.Tensor, optimizer: OptimType, learning_rate: float, eps: float,
                sparse: bool, optimizer_state: List[torch.Tensor], *tt_cores: torch.Tensor) -> torch.Tensor:
        num_tables = _num_tables(tt_p_shapes, tt_cores)
        nnz = indices.numel()
        no_cache = indices.new_empty(0)
        _, rowidx, tableidx, _, _ = _engine.preprocess_indices_sync(indices, offsets, num_tables, True, no_cache,
                                                                     no_cache.int())
        plan = _engine.make_plan(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, nnz, indices, tableidx)  # (no bag rows)
        rows = _engine.tt_rows_p(num_tables, D, tt_p_shapes, tt_q_shapes, tt_ranks, indices, tableidx, list(tt_cores), plan)
        out, argmax = _engine.bag_max_pool(rows, offsets)
        _stash(ctx, D, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer, learning_rate, eps, sparse, optimizer_state, tt_cores)
        ctx.nnz, ctx.plan = nnz, plan
        ctx.save_for_backward(indices, offsets, tableidx, argmax)
        return out.view(num_tables, B, D)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        indices, offsets, tableidx, argmax = ctx.saved_tensors
        d_rows = _engine.bag_max_pool_backward(d_output.contiguous(), argmax, offsets, ctx.nnz)
        grads = _update_cores_rows(ctx, ctx.D, ctx.nnz, indices, tableidx, d_rows)
        return _grad_tuple(TTMaxLookupFunction, len(ctx.tt_cores), grads)


class TTRowsLookupFunction(torch.autograd.Function):
    """The unpooled lookup (TTEmbedding, nn.Embedding's semantics): one row per position, no pooling launch, no bag rows.  The
    contraction runs off a plan built without bag rows (as in TTMaxLookupFunction) and writes the output buffer [N, D]
    itself; backward is the per-lookup backward / fused optimizer on the gradient rows as they come.  With `rank` (the
    positions compacted by bags_compact as N one-slot bags: `indices` holds the live ones first, `n_dev` their number on the
    device) only the live lookups are planned, contracted and trained; rows_expand / rows_collect carry the rows between the
    compacted order and the positions.  `parts` = k > 1: the geometry handed in is the core-0 row split's, `indices` hold the k
    part lookups of every position and a rows buffer [N, D] IS the parts' [k N, D / k].  Nothing is read back."""

    N_ARGS = 14

    @staticmethod
    def forward(ctx, N: int, D: int, parts: int, tt_p_shapes: List[int], tt_q_shapes: List[int], tt_ranks: List[int],
                indices: torch.Tensor, rank: Optional[torch.Tensor], n_dev: Optional[torch.Tensor], optimizer: OptimType,
                learning_rate: float, eps: float, sparse: bool, optimizer_state: List[torch.Tensor],
                *tt_cores: torch.Tensor) -> torch.Tensor:
        k = max(1, parts)
        _stash(ctx, D, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer, learning_rate, eps, sparse, optimizer_state, tt_cores)
        ctx.N, ctx.k = N, k
        if N == 0:
            ctx.plan = None
            return tt_cores[0].new_empty((0, D))
        tableidx = torch.zeros_like(indices)  # (one table)
        plan = _engine.make_plan(1, tt_p_shapes, tt_q_shapes, tt_ranks, k * N, indices, tableidx, n_dev=n_dev)  # (no bag rows)
        rows = _engine.tt_rows_p(1, D // k, tt_p_shapes, tt_q_shapes, tt_ranks, indices, tableidx, list(tt_cores), plan)
        ctx.plan = plan
        ctx.save_for_backward(indices, tableidx, rank)
        rows = rows.view(N, D)
        return rows if rank is None else _engine.rows_expand(rank, rows)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        cores = ctx.tt_cores
        if ctx.N == 0:  # an empty batch: nothing to train, zero dense gradients
            return _grad_tuple(TTRowsLookupFunction, len(cores), None if ctx.sparse else [torch.zeros_like(c) for c in cores])
        indices, tableidx, rank = ctx.saved_tensors
        N, D, k = ctx.N, ctx.D, ctx.k
        d_rows = d_output.contiguous().view(N, D)
        if rank is not None:
            d_rows = _engine.rows_collect(rank, d_rows)
        grads = _update_cores_rows(ctx, D // k, k * N, indices, tableidx, d_rows.view(k * N, D // k))
        return _grad_tuple(TTRowsLookupFunction, len(cores), grads)


class TTRowsCachedLookupFunction(torch.autograd.Function):
    """The unpooled lookup with a LIVE row cache (TTEmbedding(use_cache=True) after cache_populate()).  `indices`
    holds the n live lookups (all N positions, or -- padding dropped by bags_compact, the live count read back by the module --
    the first n of the compacted batch) and `offsets` describes them as N one-slot or empty bags (arange(N + 1), or the
    compaction's `rank`), so the bag row the live preprocess hands back for a partitioned lookup IS its position.  Forward:
    preprocess_indices_async (frequency update folded in, hits behind the misses, the split point on the device), the plan of the
    misses (make_plan(n_dev=split point), no bag rows), their contraction into scratch rows, and rows_place -- the misses' rows and
    the hits' cache rows to their positions, zeros at the padding.  Backward: rows_pick (the misses' gradient rows in partition
    order), the per-lookup backward / fused optimizer on the plan, and the cache rows' update from the gradient [N, D] itself
    with rowidx = the positions and skip_dev = the split point: SGD, row-wise Adagrad, or the dense gradient of cache_weight
    (returned in its slot).  `parts` = k > 1: the geometry handed in is the core-0 row split's; the partitioned indices are
    expanded to their k part lookups (split0_expand over `unit_offsets`, n one-lookup bags: the first k n_tt of them are the
    misses', a plan count computed on the device), and the rows [n, D] ARE the parts' [k n, D / k].
    Nothing is read back."""

    N_ARGS, CACHE_WEIGHT_ARG = 21, 19

    @staticmethod
    def forward(ctx, N: int, D: int, parts: int, tt_p_shapes: List[int], tt_q_shapes: List[int], tt_ranks: List[int],
                indices: torch.Tensor, offsets: torch.Tensor, rank: Optional[torch.Tensor], unit_offsets: Optional[torch.Tensor],
                hashtbl: torch.Tensor, cache_state: torch.Tensor, cache_freq: Optional[torch.Tensor], det: Optional[bool],
                optimizer: OptimType,
                learning_rate: float, eps: float, sparse: bool, cache_optimizer_state: Optional[torch.Tensor],
                cache_weight: torch.Tensor, optimizer_state: List[torch.Tensor], *tt_cores: torch.Tensor) -> torch.Tensor:
        k = max(1, parts)
        n = indices.numel()
        _stash(ctx, D, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer, learning_rate, eps, sparse, optimizer_state, tt_cores)
        ctx.N, ctx.n, ctx.k, ctx.det = N, n, k, det
        pcol, prow, ploc, n_tt = _engine.preprocess_indices_async(indices, offsets, hashtbl, cache_state, cache_freq)
        lookups, n_dev = pcol, n_tt
        if k > 1:
            # (unit_offsets: n one-lookup bags -- part lookups k s .. k s + k - 1 belong to partition slot s, so the misses' parts lead)
            lookups, _ = _engine.split0_expand(pcol, unit_offsets, k, tt_p_shapes[1] * tt_p_shapes[2])
            n_dev = n_tt * k
        tableidx = torch.zeros_like(lookups)  # (one table)
        plan = _engine.make_plan(1, tt_p_shapes, tt_q_shapes, tt_ranks, k * n, lookups, tableidx, n_dev=n_dev)  # (no bag rows)
        rows = _engine.tt_rows_p(1, D // k, tt_p_shapes, tt_q_shapes, tt_ranks, lookups, tableidx, list(tt_cores), plan)
        ctx.plan = plan
        ctx.save_for_backward(lookups, tableidx, prow, ploc, n_tt, cache_optimizer_state, cache_weight)
        return _engine.rows_place(N, n_tt, prow, ploc, rows.view(n, D), cache_weight, rank)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        lookups, tableidx, prow, ploc, n_tt, cache_optimizer_state, cache_weight = ctx.saved_tensors
        N, n, D, k = ctx.N, ctx.n, ctx.D, ctx.k
        d_out = d_output.contiguous().view(N, D)
        d_rows = _engine.rows_pick(n_tt, prow, d_out)[:n].view(k * n, D // k)
        grads = _update_cores_rows(ctx, D // k, k * n, lookups, tableidx, d_rows)
        d_cache_weight = _update_cache_rows(ctx, ctx.det, n, n, d_out, ploc, prow, cache_optimizer_state, cache_weight, skip_dev=n_tt)
        return _grad_tuple(TTRowsCachedLookupFunction, len(ctx.tt_cores), grads, d_cache_weight)


class TTTablesCachedLookupFunction(torch.autograd.Function):
    """The table-batched bag lookup with a LIVE row cache over several tables (TableBatchedTTEmbeddingBag(num_tables > 1,
    use_cache=True) after cache_populate()), beside TTRowsCachedLookupFunction and of its shape.  One cache
    serves all tables, keyed by key = table * key_stride + index; bags are addressed by their flat row table * B + b, the
    output and its gradient viewed as [num_tables * B, D].  Forward: table_keys, preprocess_indices_async over the keys as ONE
    table of num_tables * B bags (frequency update folded in, hits behind the misses, the split point on the device),
    table_keys_split of the misses back to (index, table, bag row), the plan of the misses (make_plan(n_dev=split point)), their
    contraction and pooling (tt_forward) and cache_forward(skip_dev=split point) for the hits.  Backward: the fused SGD /
    Adagrad or dense backward on the plan, and the cache rows' update with rowidx = the flat bag rows and skip_dev = the split
    point: SGD, row-wise Adagrad, or the dense gradient of cache_weight (returned in its slot).  Nothing is read back.
    Tables of DIFFERENT row factors (ttx_mixed.VarTableTTEmbeddingBag) run the same node: `tt_p_shapes` is then
    one list per table (cores [1, sum_k p_k_t, slice]) and `key_stride` the list of the num_tables + 1 key bases,
    key = key_stride[table] + index -- the engine's key calls take either."""

    N_ARGS, CACHE_WEIGHT_ARG = 21, 19

    @staticmethod
    def forward(ctx, B: int, D: int, num_tables: int, key_stride, tt_p_shapes: List[int], tt_q_shapes: List[int],
                tt_ranks: List[int], L: torch.Tensor, indices: torch.Tensor, offsets: torch.Tensor, hashtbl: torch.Tensor,
                cache_state: torch.Tensor, cache_freq: Optional[torch.Tensor], det: Optional[bool], optimizer: OptimType,
                learning_rate: float, eps: float, sparse: bool, cache_optimizer_state: Optional[torch.Tensor],
                cache_weight: torch.Tensor, optimizer_state: List[torch.Tensor], *tt_cores: torch.Tensor) -> torch.Tensor:
        n = indices.numel()
        _stash(ctx, D, tt_p_shapes, tt_q_shapes, tt_ranks, optimizer, learning_rate, eps, sparse, optimizer_state, tt_cores)
        ctx.B, ctx.nt, ctx.n, ctx.det = B, num_tables, n, det
        keys = _engine.table_keys(indices, offsets, num_tables, key_stride)
        pkey, prow, ploc, n_tt = _engine.preprocess_indices_async(keys, offsets, hashtbl, cache_state, cache_freq)
        # (prow: the flat bag row table * B + b -- the preprocess saw one table of num_tables * B bags)
        idx, tableidx, rowidx = _engine.table_keys_split(pkey, prow, num_tables, B, key_stride, n_dev=n_tt)
        plan = _engine.make_plan(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, n, idx, tableidx, rowidx, n_dev=n_tt)
        output = _engine.tt_forward(1000, num_tables, B, D, tt_p_shapes, tt_q_shapes, tt_ranks, L, n, idx, rowidx, tableidx,
                                    list(tt_cores), plan=plan)
        _engine.cache_forward(num_tables * B, n, ploc, prow, cache_weight, output, skip_dev=n_tt)
        ctx.plan = plan
        ctx.save_for_backward(L, idx, rowidx, tableidx, prow, ploc, n_tt, cache_optimizer_state, cache_weight)
        return output

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        L, idx, rowidx, tableidx, prow, ploc, n_tt, cache_optimizer_state, cache_weight = ctx.saved_tensors
        n = ctx.n
        d_output = d_output.contiguous()
        d_flat = d_output.view(ctx.nt * ctx.B, ctx.D)
        grads = _update_cores_bags(ctx, L, n, idx, rowidx, tableidx, d_output)
        d_cache_weight = _update_cache_rows(ctx, ctx.det, n, n, d_flat, ploc, prow, cache_optimizer_state, cache_weight, skip_dev=n_tt)
        return _grad_tuple(TTTablesCachedLookupFunction, len(ctx.tt_cores), grads, d_cache_weight)


class _RowsAtPositionsFunction(torch.autograd.Function):
    """rows_expand / rows_collect around a lookup that returned the rows of the live positions only (TTEmbedding's dedup route
    with padding_idx, where the live count n has been read back): rows [n, D] -> out [N, D], zeros at the padding."""

    @staticmethod
    def forward(ctx, rows: torch.Tensor, rank: torch.Tensor) -> torch.Tensor:
        ctx.save_for_backward(rank)
        ctx.n = rows.size(0)
        N = rank.numel() - 1
        full = rows.new_empty((N, rows.size(1)))  # (rows_expand reads the rows of live positions only: the first n)
        full[:ctx.n].copy_(rows)
        return _engine.rows_expand(rank, full)

    @staticmethod
    def backward(ctx, d_output: torch.Tensor):
        (rank,) = ctx.saved_tensors
        return _engine.rows_collect(rank, d_output.contiguous())[:ctx.n], None


# --------------------------------------------------------------------------- #
# shape factoring (init-time helper; reference :359-418)
# --------------------------------------------------------------------------- #

def _prime_factors(n: int) -> Dict[int, int]:
    out: Dict[int, int] = {}
    f = 2
    while f * f <= n:
        while n % f == 0:
            out[f] = out.get(f, 0) + 1
            n //= f
        f += 1 if f == 2 else 2
    if n > 1:
        out[n] = out.get(n, 0) + 1
    return out


def _entropy(xs: Sequence[int]) -> float:
    v = np.asarray(xs, dtype=np.float64)
    pk = v / v.sum()
    pk = pk[pk > 0]
    return float(-(pk * np.log(pk)).sum())


def _balanced_factors(n: int, d: int) -> List[int]:
    """The factorisation of n into d factors with maximal entropy of the
    normalised factors, listed small/large interleaved like the reference."""
    primes = _prime_factors(n)
    splits = []  # per prime: all ways to spread its exponent over d ordered bins
    for prime, e in primes.items():
        ways = []
        for cuts in itertools.combinations(range(e + d - 1), d - 1):
            prev, exps = -1, []
            for c in cuts + (e + d - 1,):
                exps.append(c - prev - 1)
                prev = c
            ways.append([prime ** k for k in exps])
        splits.append(ways)
    seen = set()
    for combo in itertools.product(*splits) if splits else [()]:
        bins = [1] * d
        for way in combo:
            bins = [b * w for b, w in zip(bins, way)]
        seen.add(tuple(sorted(bins)))
    best = max(sorted(seen), key=_entropy)
    lo, hi = list(best[: d // 2]), list(best[d // 2:])
    out: List[int] = []
    for a, b in itertools.zip_longest(lo, hi):
        if a is not None:
            out.append(a)
        if b is not None:
            out.append(b)
    return out


def suggested_tt_shapes(n: int, d: int = 3, allow_round_up: bool = True) -> List[int]:
    n = int(n)
    if not allow_round_up:
        return _balanced_factors(n, d)
    candidates = []
    for k in range(len(str(n))):
        step = 10 ** k
        candidates.append(_balanced_factors(-(-n // step) * step, d))
    return candidates[int(np.argmax([_entropy(c) for c in candidates]))]


# --------------------------------------------------------------------------- #
# modules
# --------------------------------------------------------------------------- #

def _check_module_kwargs(cls, kw: dict) -> None:
    """from_pretrained's `module_kwargs` against `cls`'s constructor, before the (long) factorisation: a TypeError for a keyword
    it does not take (`freeze`: the modules train) or that from_pretrained sets itself"""
    import inspect

    own = ("self", "num_tables", "num_embeddings", "embedding_dim", "tt_ranks", "tt_p_shapes", "tt_q_shapes")
    known = [n for n in inspect.signature(cls.__init__).parameters if n not in own]
    for name in kw:
        if name not in known:
            raise TypeError(f"{cls.__name__}.from_pretrained() got an unexpected keyword argument {name!r}")


class TableBatchedTTEmbeddingBag(nn.Module):
    """`num_tables` TT-compressed embedding tables of identical shape looked up
    in one pass (sum pooling -- or `mode="mean"` / `"max"` --, include_last_offset form: offsets has
    num_tables*B + 1 entries, bags ordered table-major).  `use_cache=True` with several tables (not in the reference): ONE LFU
    row cache over all of them, keyed by table * prod(tt_p_shapes) + index."""

    __constants__ = ["num_tables", "num_embeddings", "embedding_dim", "tt_shape", "tt_rank"]

    def __init__(self, num_tables: int, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, use_cache: bool = False, cache_size: int = 0, hashtbl_size: int = 0,
                 weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 device: Optional[torch.device] = None, include_last_offset: bool = True, dedup: bool = False,
                 reference_exact_populate: bool = False, deterministic_cache_update: Optional[bool] = None,
                 mode: str = "sum", padding_idx: Optional[int] = None, betas: Tuple[float, float] = (0.9, 0.999),
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False) -> None:
        super().__init__()
        # betas, weight_decay, decoupled_weight_decay (trailing keywords, not in the reference): read under
        # optimizer=OptimType.EXACT_ADAM only -- torch.optim.Adam's (decoupled_weight_decay=True: AdamW's) step on all cores inside
        # backward, `learning_rate` and `eps` being the existing arguments (`_init_adam`)
        # mode (trailing keyword, not in the reference): nn.EmbeddingBag's pooling -- "sum" (the reference's, the default here),
        # "mean" (the bag sum over the bag length: a per-bag scale around the sum lookup, every route) or "max" (column-wise max,
        # the gradient to the winning lookup only: rows, max pool and a per-lookup backward; no live cache, no dedup, no n_dev)
        if mode not in POOLING_MODES:
            raise ValueError(f"mode must be one of {POOLING_MODES}, got {mode!r}")
        if mode == "max" and use_cache:
            raise NotImplementedError("mode='max' does not support use_cache=True (the cache rows are pooled by sum)")
        if mode == "max" and dedup:
            raise NotImplementedError("mode='max' does not support dedup (duplicate lookups would share one winning row)")
        self.mode = mode
        # padding_idx (trailing keyword, not in the reference): nn.EmbeddingBag's -- lookups of this index (the same value in every
        # table) contribute nothing to their bag, receive no gradient and are not counted by the cache's frequency table; a bag of
        # padding only is zero in every mode.  The slots are dropped on the device in front of the lookup (include/ttx.h "padded
        # bags"), so they cost no contraction.  A TT table holds no independent zero row: full_weight()[padding_idx] is whatever
        # the cores give, it is just never looked up through a padded call.
        self.padding_idx = _normalise_padding_idx(padding_idx, int(num_embeddings))
        # deterministic_cache_update (trailing keyword, not in the reference): how the backward updates the CACHE rows.  True: the
        # cached lookups are grouped by cache row with a stable sort, a row's bag gradients added in index order, one writer per row --
        # cache_weight (and the row-wise Adagrad state) bit-identical from run to run (ttx_cache_backward_sorted).  False: the
        # reference's formulation, float atomics in one launch -- the last bits depend on arrival order.  None: sorted from 262,144
        # lookups per batch on (row-wise Adagrad: 65,536), where it is also the faster of the two.  The TT
        # cores' update never uses atomics.
        self.deterministic_cache_update = deterministic_cache_update
        # reference_exact_populate (trailing keyword, not in the reference): cache_populate() leaves the cache_state of evicted
        # slots untouched, bit for bit what the reference's mark_popular_colidx_kernel does (cu:1131-1133).  Default False: an
        # evicted slot drops its cache row (deviation 5).  Carried per call (TTX_POPULATE_REFERENCE_EXACT);
        # rounds 3-5 had a process-wide switch for it.
        self.reference_exact_populate = bool(reference_exact_populate)
        # dedup (not in the reference): lookups of a batch that repeat a (table, row) pair share ONE contraction,
        # forward and backward (include/ttx.h "duplicate lookups").  Same results; pays on skewed index streams
        # while the row cache is not live, costs the key sort and two extra launches on uniform ones.
        # dedup="auto": the module decides per batch -- sharing runs only at batches of >= _DEDUP_AUTO_MIN_NNZ lookups
        # (below that every kernel of the plain step sits at its launch floor: sharing cannot pay) and only
        # while the stream's last sampled batch had <= _DEDUP_AUTO_MAX_DISTINCT distinct pairs per lookup; the sample is
        # the shared path itself (its map holds the distinct count; one read-back every _DEDUP_AUTO_PERIOD batches, never
        # under stream capture).
        self.dedup = "auto" if dedup == "auto" else bool(dedup)
        self._dd_auto = [False, 0]  # [sharing on, batches until the next sample]
        # nn.EmbeddingBag call form: False = offsets hold only the bag starts (PyTorch's default,
        # what DLRM passes); True = the reference's form, num_tables*B + 1 entries (:851)
        self.include_last_offset = bool(include_last_offset)
        if device is None:
            if not torch.cuda.is_available():
                raise RuntimeError("TTEmbeddingBag needs a GPU (the reference asserts torch.cuda.is_available(), :454)")
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        num_embeddings, embedding_dim = int(num_embeddings), int(embedding_dim)
        assert num_tables > 0 and num_embeddings > 0 and embedding_dim > 0
        tt_ranks = [int(x) for x in tt_ranks]
        nd = len(tt_ranks) + 1
        self.tt_p_shapes: List[int] = [int(x) for x in tt_p_shapes] if tt_p_shapes is not None \
            else suggested_tt_shapes(num_embeddings, nd)
        self.tt_q_shapes: List[int] = [int(x) for x in tt_q_shapes] if tt_q_shapes is not None \
            else suggested_tt_shapes(embedding_dim, nd, allow_round_up=not enforce_embedding_dim)
        assert 2 <= len(self.tt_p_shapes) <= 4
        assert len(self.tt_p_shapes) == nd == len(self.tt_q_shapes)
        assert all(v > 0 for v in self.tt_p_shapes + self.tt_q_shapes + tt_ranks)
        assert int(np.prod(np.asarray(self.tt_p_shapes, dtype=np.int64))) >= num_embeddings
        assert int(np.prod(np.asarray(self.tt_q_shapes, dtype=np.int64))) == embedding_dim
        self.num_tables, self.tt_ndim = num_tables, nd
        self.num_embeddings, self.embedding_dim = num_embeddings, embedding_dim
        self.tt_ranks = [1] + tt_ranks + [1]
        self._split0 = _split0_factor(self.tt_q_shapes, tt_ranks)  # (q0 > 4: part lookups on the q0 <= 4 kernels)
        self._pad0 = _pad0_target(self.tt_q_shapes, tt_ranks)       # (... of core 0 padded to a multiple of 4 slots, round 4)
        if self._pad0:
            self._split0 = self._pad0 // 4
        if self._split0 > 1 and getattr(_engine, "debug_tiles", None) is not None and not isinstance(self.tt_p_shapes[0], (list, tuple)):
            # ... if the engine has a specialised kernel for the PART geometry (a padded template may be refused for wasting
            # more than 8x its work, the specialised kernels may be switched off): k times the lookups on the generic kernels
            # would be slower than the unsplit table on them (round 3 advisor)
            try:
                k = self._split0
                part = _engine.debug_tiles(num_tables, [k * self.tt_p_shapes[0]] + list(self.tt_p_shapes[1:]),
                                           [(self._pad0 or self.tt_q_shapes[0]) // k] + list(self.tt_q_shapes[1:]), list(self.tt_ranks))
                if part["MC"] != 0:
                    self._split0 = self._pad0 = 0
            except Exception:  # noqa: BLE001 -- the query is advice, never a reason to fail construction
                pass
        self.sparse, self.optimizer, self.learning_rate, self.eps = sparse, optimizer, learning_rate, eps
        logging.info("Creating TTEmbeddingBag tt_p_shapes: %s, tt_q_shapes: %s, tt_ranks: %s, sparse: %s, "
                     "optimizer: %s, learning_rate: %s, eps: %s, use_cache: %s, cache_size: %s, hashtbl_size: %s",
                     self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, sparse, optimizer, learning_rate, eps,
                     use_cache, cache_size, hashtbl_size)
        strides = [int(np.prod(np.asarray(self.tt_p_shapes[t + 1:], dtype=np.int64))) for t in range(nd)]
        self.register_buffer("L", torch.tensor(strides, dtype=torch.int64, device=device))
        self.tt_cores = nn.ParameterList()
        self.optimizer_state = BufferList("optimizer_state")
        stateful = optimizer not in _SGD_LIKE and (sparse or optimizer != OptimType.EXACT_ADAM)  # (Adam's state: with sparse=True only)
        for t in range(nd):
            shape = (num_tables, self.tt_p_shapes[t], self.tt_ranks[t] * self.tt_q_shapes[t] * self.tt_ranks[t + 1])
            self.tt_cores.append(nn.Parameter(torch.empty(shape, device=device, dtype=torch.float32)))
            self.optimizer_state.append(torch.zeros(shape if stateful else 0, device=device, dtype=torch.float32))
        self._init_adam(betas, weight_decay, decoupled_weight_decay, use_cache)
        self.reset_parameters(weight_dist)
        self.use_cache = use_cache
        if use_cache:
            # num_tables > 1 (not in the reference, whose cache serves one table, :456): ONE cache over all tables, keyed by
            # table * key_stride + index with key_stride = prod(tt_p_shapes) -- the cache_size hottest rows across the tables
            # (DESIGN.md 4.13).  Same parameters, buffers and state_dict() keys as the one-table cached module.
            cache_size = cache_size if cache_size > 0 else int(0.1 * num_tables * num_embeddings)
            hashtbl_size = hashtbl_size if hashtbl_size > 0 else num_tables * num_embeddings
            if num_tables > 1:
                if hashtbl_size >= 2 ** 31:
                    raise ValueError(f"hashtbl_size must stay below 2^31, got {hashtbl_size} (the default is num_tables * "
                                     f"num_embeddings: pass a smaller hashtbl_size)")
                if num_tables * self._key_stride() >= 2 ** 62:
                    raise ValueError(f"the cache's key space num_tables * prod(tt_p_shapes) = {num_tables} * {self._key_stride()} "
                                     f"does not fit 2^62")
            assert hashtbl_size >= cache_size
            self.register_buffer("hashtbl", torch.full((hashtbl_size,), -1, device=device, dtype=torch.int64))
            self.register_buffer("cache_freq", torch.zeros(hashtbl_size, device=device, dtype=torch.int64))
            self.register_buffer("cache_state", torch.full((hashtbl_size,), -1, device=device, dtype=torch.int32))
            self.cache_weight = nn.Parameter(torch.zeros((cache_size, embedding_dim), device=device, dtype=torch.float32))
            if sparse and stateful:
                shape = (cache_size, embedding_dim) if optimizer == OptimType.EXACT_ADAGRAD else (cache_size,)
                self.register_buffer("cache_optimizer_state", torch.zeros(shape, device=device, dtype=torch.float32))
            else:
                self.cache_optimizer_state = None
        else:
            self.register_buffer("hashtbl", torch.empty(0, device=device, dtype=torch.int64))
            self.register_buffer("cache_state", torch.empty(0, device=device, dtype=torch.int32))
            self.cache_optimizer_state = None
            self.cache_weight = None
        self.warmup = True

    # ------------------------------------------------------- OptimType.EXACT_ADAM
    def _init_adam(self, betas, weight_decay: float, decoupled: bool, use_cache: bool) -> None:
        """called by the constructors once tt_cores / optimizer_state exist.  Under sparse=True and OptimType.EXACT_ADAM:
        `optimizer_state{t}` is exp_avg, the second BufferList `optimizer_state_v` exp_avg_sq (both in the core's shape) and the
        buffer `optimizer_step` int64 [1] the steps taken.  Every other module gets no new buffer: its state_dict() is unchanged."""
        self._adam = None
        if not (self.sparse and self.optimizer == OptimType.EXACT_ADAM):
            return
        if use_cache:
            # (cached rows would need per-row moments that move with the rows in cache_populate(keep_trained=): a piece of its own)
            raise NotImplementedError("OptimType.EXACT_ADAM does not support use_cache=True (the cache rows have no Adam state)")
        b1, b2, wd = _check_adam_args(betas, weight_decay)
        self._adam = (b1, b2, wd, bool(decoupled))
        self.optimizer_state_v = BufferList("optimizer_state_v", [torch.zeros_like(s) for s in self.optimizer_state])
        self.register_buffer("optimizer_step", torch.zeros(1, dtype=torch.int64, device=self.tt_cores[0].device))

    def _route_args(self, live: bool = True):
        """-> (sparse, cores) as the lookup routes see them.  Under OptimType.EXACT_ADAM: (False, the cores passed through
        _AdamStepFunction) -- every route runs as for sparse=False, and the dense core gradients end in ONE Adam step per backward.
        `live` False: the batch is empty, backward takes no step."""
        if self.__dict__.get("_adam") is None:
            return self.sparse, self.tt_cores
        return False, list(_AdamStepFunction.apply(self, live, *self.tt_cores))

    def _adam_step_from(self, grads) -> None:
        _adam_step([p.detach() for p in self.tt_cores], grads, list(self.optimizer_state), list(self.optimizer_state_v),
                   self.optimizer_step, self.learning_rate, self.eps, self._adam)

    # ------------------------------------------------------------------ init
    def full_weight(self, table: Optional[int] = None) -> torch.Tensor:
        """`table` None: the one table of a one-table module expanded to [prod(tt_p_shapes), D] (the reference's).  An integer (not
        in the reference): that table's [num_embeddings, D], of any number of tables."""
        if table is not None:
            return _svd.tt_full(self.table_cores(table), self.num_embeddings)
        assert self.num_tables == 1, "full_weight() only supported for num_tables == 1 for now"
        return tt_matrix_to_full(self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, list(self.tt_cores), [1, 0, 2, 3])

    # ------------------------------------------------- canonical cores, from_pretrained, truncate_ranks
    def _table_index(self, table: int) -> int:
        if isinstance(table, bool) or not hasattr(table, "__index__") or not -self.num_tables <= int(table) < self.num_tables:
            raise IndexError(f"table {table!r}: the module has {self.num_tables} table(s)")
        return int(table) % self.num_tables

    def table_cores(self, table: int = 0) -> List[torch.Tensor]:
        """one table's cores in the layout-independent CANONICAL form of ttx_svd: core k [r_k, p_k, q_k, r_{k+1}], copies"""
        k = self._table_index(table)
        return _svd.from_module_layout([c.detach()[k] for c in self.tt_cores], self.tt_q_shapes, self.tt_ranks)

    def _check_loadable(self, cores, p: Sequence[int], q: Sequence[int], ranks: Sequence[int], exact: bool) -> List[int]:
        """canonical `cores` against one table's geometry -> their [r_0 .. r_T]; `exact`: the ranks must be `ranks`, else at most"""
        if len(cores) != len(p):
            raise ValueError(f"{len(p)} cores expected, got {len(cores)}")
        got = _svd._check_cores(cores)
        for t, c in enumerate(cores):
            if int(c.size(1)) != p[t] or int(c.size(2)) != q[t]:
                raise ValueError(f"core {t}: expected [r, {p[t]}, {q[t]}, r'], got {list(c.shape)}")
        if (got != list(ranks)) if exact else any(a > b for a, b in zip(got, ranks)):
            raise ValueError(f"the cores' ranks {got[1:-1]} do not fit the module's {list(ranks)[1:-1]}")
        if self.use_cache and not self.warmup:
            raise RuntimeError("load_table_cores with a live cache: the cached rows would no longer belong to the cores "
                               "(reset_cache() first)")
        return got

    def load_table_cores(self, cores: Sequence[torch.Tensor], table: int = 0) -> None:
        """write one table's cores from the canonical form (`table_cores`' / ttx_svd's), shapes checked; optimizer state and
        cache are left as they are (a live cache is refused)"""
        k = self._table_index(table)
        self._check_loadable(cores, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, exact=True)
        with torch.no_grad():
            for dst, src in zip(self.tt_cores, _svd.to_module_layout(cores)):
                dst[k].copy_(src)

    _STACKED_TABLES = True  # from_pretrained takes [num_tables, E, D] (the one-table modules: [E, D])

    @classmethod
    def _construct(cls, num_embeddings, embedding_dim: int, tt_ranks, tt_p_shapes, tt_q_shapes, kw: dict):
        """the ordinary constructor behind from_pretrained / truncate_ranks; `num_embeddings`: one cardinality per table"""
        return cls(len(num_embeddings), num_embeddings[0], embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, **kw)

    @staticmethod
    def _pretrained_tables(embeddings, stacked: bool) -> List[torch.Tensor]:
        """`embeddings` -> one [E, D] tensor per table, checked (ValueError) before any arithmetic"""
        if isinstance(embeddings, torch.Tensor):
            if embeddings.dim() != (3 if stacked else 2):
                raise ValueError(f"embeddings: a tensor {'[num_tables, E, D] or a list of [E, D]' if stacked else '[E, D]'}, "
                                 f"got {list(embeddings.shape)}")
            tables = list(embeddings.unbind(0)) if stacked else [embeddings]
        else:
            tables = list(embeddings)
        if not tables or any(not isinstance(w, torch.Tensor) or w.dim() != 2 or not w.is_floating_point() for w in tables):
            raise ValueError("embeddings: 2-D floating-point tables [E, D]")
        if len({int(w.size(1)) for w in tables}) != 1:
            raise ValueError("embeddings: every table needs the same embedding dimension")
        return tables

    @staticmethod
    def _pretrained_dims(tt_ranks, tt_p_shapes, tt_q_shapes) -> int:
        """the number of cores from_pretrained factors into: what the given ranks / shapes say, else the constructors' three"""
        for v, extra in ((tt_ranks, 1), (tt_p_shapes, 0), (tt_q_shapes, 0)):
            if v is not None:
                return len(v) + extra
        return 3

    @classmethod
    def from_pretrained(cls, embeddings, tt_ranks: Optional[Sequence[int]] = None, tt_p_shapes: Optional[List[int]] = None,
                        tt_q_shapes: Optional[List[int]] = None, *, rel_error: Optional[float] = None,
                        max_rank: Optional[int] = None, rank_multiple: int = 1, **module_kwargs):
        """nn.EmbeddingBag.from_pretrained's counterpart (not in the reference): the module whose tables are the
        TT-SVD (ttx_svd.tt_svd) of the dense tables `embeddings` -- [num_tables, E, D] or a list of [E, D] for the batched module,
        [E, D] for the one-table modules.  `tt_ranks`: the module's ranks, exactly (`rel_error` / `max_rank` / `rank_multiple`
        instead: chosen per table for ||W - TT||_F <= rel_error ||W||_F, the module built at the per-position maximum and every
        table zero-padded to it).  `tt_p_shapes` / `tt_q_shapes` default as in the constructor; `module_kwargs` are the
        constructor's (optimizer, sparse, use_cache, mode, padding_idx, device, ...).  The factorisation runs where `embeddings`
        lives.  The module is built by its constructor -- optimizer state zero, a cache in warm-up -- and its cores are loaded;
        `module.compression` lists (ranks, bound, norm) per table.  There is no `freeze`: the result trains like any module."""
        _check_module_kwargs(cls, module_kwargs)
        tables = cls._pretrained_tables(embeddings, stacked=cls._STACKED_TABLES)
        if len({int(w.size(0)) for w in tables}) != 1:
            raise ValueError("embeddings: the tables of a batched module share one shape (ttx_mixed.VarTableTTEmbeddingBag: any)")
        E, D = int(tables[0].size(0)), int(tables[0].size(1))
        nd = cls._pretrained_dims(tt_ranks, tt_p_shapes, tt_q_shapes)
        p = [int(x) for x in tt_p_shapes] if tt_p_shapes is not None else suggested_tt_shapes(E, nd)
        q = [int(x) for x in tt_q_shapes] if tt_q_shapes is not None \
            else suggested_tt_shapes(D, nd, allow_round_up=not module_kwargs.get("enforce_embedding_dim", False))
        res = [_svd.tt_svd(w, p, q, tt_ranks, rel_error=rel_error, max_rank=max_rank, rank_multiple=rank_multiple) for w in tables]
        return cls._from_factors(res, [E] * len(tables), D, p, q, module_kwargs)

    @classmethod
    def _from_factors(cls, res, num_embeddings, D: int, p, q, kw: dict):
        ranks = _svd.merged_ranks(res)
        kw = dict(kw)
        kw.setdefault("weight_dist", "uniform")  # (the cheapest initialiser: the cores are overwritten)
        m = cls._construct(num_embeddings, D, ranks, p, q, kw)
        for k, r in enumerate(res):
            m.load_table_cores(_svd.tt_pad_ranks(r.cores, ranks), k)
        m.compression = [(list(r.ranks), r.bound, r.norm) for r in res]
        return m

    def _ctor_kwargs(self) -> dict:
        """the constructor's keywords as this module was built (ranks and shapes apart)"""
        adam = self.__dict__.get("_adam") or (0.9, 0.999, 0.0, False)
        kw = dict(optimizer=self.optimizer, learning_rate=self.learning_rate, eps=self.eps, sparse=self.sparse,
                  use_cache=bool(self.use_cache), device=self.tt_cores[0].device, include_last_offset=self.include_last_offset,
                  dedup=self.dedup, reference_exact_populate=self.reference_exact_populate,
                  deterministic_cache_update=self.deterministic_cache_update, mode=self.mode, padding_idx=self.padding_idx,
                  betas=(adam[0], adam[1]), weight_decay=adam[2], decoupled_weight_decay=adam[3])
        if self.use_cache:
            kw.update(cache_size=int(self.cache_weight.size(0)), hashtbl_size=int(self.hashtbl.numel()))
        return kw

    def truncate_ranks(self, new_ranks: Optional[Sequence[int]] = None, *, rel_error: Optional[float] = None,
                       max_rank: Optional[int] = None, rank_multiple: int = 1):
        """-> a NEW module of the same constructor arguments at lower TT ranks (not in the reference): every table
        rounded by ttx_svd.tt_round -- to `new_ranks`, or per table for `rel_error` (the module at the per-position maximum).
        Not in place: the Parameters' shapes and the registered state change with the ranks.  Optimizer state starts at zero; a
        LIVE cache is refused (its rows would no longer belong to the cores: reset_cache() first); `compression` as
        from_pretrained's, against the tables this module holds."""
        if self.use_cache and not self.warmup:
            raise RuntimeError("truncate_ranks with a live cache: the cached rows would no longer belong to the cores "
                               "(reset_cache() first)")
        res = [_svd.tt_round(self.table_cores(k), new_ranks, rel_error=rel_error, max_rank=max_rank, rank_multiple=rank_multiple)
               for k in range(self.num_tables)]
        return type(self)._from_factors(res, [self.num_embeddings] * self.num_tables, self.embedding_dim, list(self.tt_p_shapes),
                                        list(self.tt_q_shapes), self._ctor_kwargs())

    def _assign(self, t: int, values: np.ndarray) -> None:
        core = self.tt_cores[t]
        with torch.no_grad():
            core.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).reshape(core.shape))

    def reset_parameters(self, weight_dist: str) -> None:
        """The five initialisations of the reference (:613-792)."""
        nd, E, D = self.tt_ndim, self.num_embeddings, self.embedding_dim
        if weight_dist == "uniform":
            sigma = math.sqrt(2.0 / (E + D))
            shrink = float(np.prod(np.asarray(self.tt_ranks, dtype=np.float64) ** (-1.0 / (2 * nd))))
            hi = sigma ** (1.0 / nd) * shrink
            for core in self.tt_cores:
                nn.init.uniform_(core, 0.0, hi)
        elif weight_dist == "naive-uniform":
            for core in self.tt_cores:
                nn.init.uniform_(core, 0.0, 1.0 / math.sqrt(E))
        elif weight_dist == "normal":
            for core in self.tt_cores:
                nn.init.normal_(core, 0.0, 1.0 / math.sqrt(E))
                with torch.no_grad():
                    core.mul_(1.0 / self.tt_ranks[0])
        elif weight_dist == "approx-normal":
            # N(0,1) truncated to |x| >= 2 by rejection, scaled by (3E)^(-1/6).  The reference redraws entry after
            # entry (:650-654): the j-th rejected entry ends up with the j-th accepted value of the stream that
            # follows the first draw.  Done here in blocks -- each block draws exactly as many values as are still
            # missing, so the stream is consumed to the same point and every entry gets the same value.
            scale = (1.0 / math.sqrt(3 * E)) ** (1.0 / 3.0)
            for t, core in enumerate(self.tt_cores):
                w = np.random.normal(0.0, 1.0, size=tuple(core.shape)).astype(np.float32).ravel()
                small = np.flatnonzero(np.abs(w) < 2)
                done = 0
                while done < small.size:
                    x = np.random.normal(0.0, 1.0, size=small.size - done).astype(np.float32)
                    x = x[np.abs(x) >= 2]
                    w[small[done:done + x.size]] = x
                    done += x.size
                self._assign(t, w * np.float64(scale))  # (float64 product, rounded once: `W *= scale` with a numpy scalar)
        elif weight_dist == "approx-uniform":
            self._init_approx_uniform()
        else:
            raise AssertionError(f"unknown weight_dist {weight_dist!r}")

    def _init_approx_uniform(self, sigma: float = 0.01, gridpts: int = 15, width: float = 0.7 / 30.0) -> None:
        """'flat saw-tooth' construction (:660-792): the product of the three
        cores is a train of narrow teeth j/gridpts + U(-width/2, width/2) that
        a narrow Gaussian smears into a uniform density.  3 cores, 1 table."""
        assert self.tt_ndim == 3, "approx-uniform needs exactly 3 TT cores"
        assert self.num_tables == 1, "approx_uniform only supported for num_tables == 1"
        r, p, q = self.tt_ranks, self.tt_p_shapes, self.tt_q_shapes
        scale = 1.0 / (math.sqrt(self.num_embeddings) ** (1.0 / 3.0))

        def teeth(count: int) -> np.ndarray:
            j = np.random.randint(-(gridpts - 1), gridpts, count)
            return j * (1.0 / gridpts) + (-width / 2.0 + width * np.random.rand(count))

        # head: all entries ~ N(1/sqrt(r1), sigma)
        head = (1.0 / math.sqrt(r[1])) + np.random.randn(r[0], p[0], q[0], r[1]) * sigma
        # middle: ~ N(1/sqrt(r1), sigma); per (m, n) one even column k is made tiny except one tooth entry
        mid_scale = 1.0 / math.sqrt(r[1])
        mid = (mid_scale + np.random.randn(r[1], p[1] * q[1], r[2]) * sigma)
        vals = teeth(p[1] * q[1]) / mid_scale
        for ell in range(p[1] * q[1]):
            k = random.randrange(0, r[2], 2)
            mid[:, ell, k] = np.random.randn(r[1]) * (sigma * sigma / mid_scale)
            mid[random.randrange(r[1]), ell, k] = vals[ell]
        mid = mid.reshape(r[1], p[1], q[1], r[2])
        # tail: small background, per (m, n) one odd row carries a tooth
        tail = (np.random.randn(r[2], p[2] * q[2]) * sigma)
        vals = teeth(p[2] * q[2])
        for ell in range(p[2] * q[2]):
            tail[random.randrange(1, r[2], 2) if r[2] > 1 else 0, ell] = vals[ell]
        tail = tail.reshape(r[2], p[2], q[2], r[3])
        for t, w in enumerate((head, mid, tail)):
            self._assign(t, (w * scale).transpose(1, 0, 2, 3).reshape(1, p[t], -1))

    # ----------------------------------------------------------------- cache
    def reset_cache(self) -> None:
        if self.use_cache:
            self.hashtbl.fill_(-1)
            self.cache_freq.fill_(0)
            self.cache_state.fill_(-1)
            self.warmup = True
            self._drop_prefetched(counted=False)  # (the frequency table is empty again)

    @torch.no_grad()
    def _write_back(self, lr: float, steps: int = 1) -> None:
        """`steps` SGD steps of size `lr` on the cores toward every CACHED row (see cache_populate).  Plain SGD whatever the
        module's optimizer (a correction of the cores toward the cached rows, not a training step: Adagrad's accumulators are not
        touched); batches planned ahead hold no plan of the cores' VALUES (plans are index work), so they stay valid."""
        slots = torch.nonzero(self.cache_state >= 0).flatten()
        n = int(slots.numel())
        if n == 0:
            return
        keys = self.hashtbl[slots].contiguous()
        target = self.cache_weight.detach()[self.cache_state[slots].long()]           # what the cached rows have learnt
        offsets = torch.arange(0, n + 1, dtype=torch.int64, device=keys.device)     # one lookup per bag
        no_tbl = torch.empty(0, dtype=torch.int64, device=keys.device)
        colidx, rowidx, tableidx, _, _ = _engine.preprocess_indices_sync(keys, offsets, 1, True, no_tbl,
                                                                          torch.empty(0, dtype=torch.int32, device=keys.device))
        cores = [c.detach() for c in self.tt_cores]
        for _ in range(max(1, int(steps))):
            rows = _engine.tt_forward(1000, 1, n, self.embedding_dim, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, self.L, n,
                                      colidx, rowidx, tableidx, cores)                  # the rows as the cores hold them
            diff = (rows - target.unsqueeze(0)).contiguous()  # d/d row of 1/2 ||TT row - cached row||^2
            _engine.tt_sgd_backward(1000, self.embedding_dim, float(lr), self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, self.L,
                                    n, colidx, rowidx, tableidx, diff, cores)

    def _key_stride(self) -> int:
        """the row cache over several tables keys a lookup by table * key_stride + index: prod(tt_p_shapes), the range the
        index decode covers (>= num_embeddings)"""
        return int(np.prod(np.asarray(self.tt_p_shapes, dtype=np.int64)))

    def _key_space(self):
        """what the key calls take in the place of `key_stride`: the one stride -- or, where a subclass batches tables of different
        row factors, the list of its num_tables + 1 key bases (ttx_mixed.VarTableTTEmbeddingBag)"""
        return self._key_stride()

    def _tables_cache(self) -> bool:
        """one row cache over several tables"""
        return bool(self.use_cache) and self.num_tables > 1

    def _count_keys(self, indices: torch.Tensor, offsets: torch.Tensor) -> None:
        """several tables: the frequency table counts KEYS (offsets with their closing entry) -- one launch on the GPU
        (table_keys with the count folded in), torch ops on CPU tensors (the tests' oracle engine)."""
        if indices.numel() == 0:
            return
        space = self._key_space()
        if indices.is_cuda and getattr(_engine, "table_keys", None) is not None:
            _engine.table_keys(indices, offsets, self.num_tables, space, self.hashtbl, self.cache_freq)
            return
        B = (offsets.numel() - 1) // self.num_tables
        bounds = offsets[::B][1:self.num_tables].contiguous()  # the first position of tables 1 .. num_tables - 1
        table = torch.bucketize(torch.arange(indices.numel(), dtype=torch.int64, device=indices.device), bounds, right=True)
        if isinstance(space, (list, tuple)):  # (key bases: one per table)
            first = torch.tensor(list(space[:-1]), dtype=torch.int64, device=indices.device)[table]
        else:
            first = table * space
        _engine.update_cache_state((indices + first).contiguous(), self.hashtbl, self.cache_freq)

    def _refresh_check(self, keep_trained: bool, freq_shift: int) -> None:
        """what cache_populate(keep_trained=, freq_shift=) refuses -- before anything is changed"""
        if isinstance(freq_shift, bool) or not hasattr(freq_shift, "__index__") or not 0 <= int(freq_shift) < 63:
            raise ValueError(f"cache_populate(freq_shift={freq_shift!r}): an integer in [0, 63)")
        if keep_trained and self.use_cache:
            if self.reference_exact_populate:
                raise ValueError("cache_populate(keep_trained=True) reads the cache_state of every slot, and with "
                                 "reference_exact_populate=True evicted slots keep stale ones: use one or the other")
            if getattr(_engine, "cache_carry", None) is None or not self.cache_weight.is_cuda:
                raise NotImplementedError("cache_populate(keep_trained=True) moves the rows on the GPU only")

    def _refresh_begin(self, keep_trained: bool, freq_shift: int):
        """in front of the populate's sort: age the frequencies (cache_freq >>= freq_shift) and, for keep_trained on a live
        cache, copy what the populate overwrites -> (cache_state, cache_weight, state or None) as they were, or None"""
        if not self.use_cache:
            return None
        if int(freq_shift) > 0:
            self.cache_freq.bitwise_right_shift_(int(freq_shift))
        if not keep_trained or self.warmup:  # (still warming up: no row has been trained)
            return None
        state = self._cache_row_state()
        return self.cache_state.clone(), self.cache_weight.detach().clone(), None if state is None else state.clone()

    def _cache_row_state(self) -> Optional[torch.Tensor]:
        """the cache rows' optimizer state as the update kernels use it: ONE float per row, the first cache_size floats of the
        buffer whatever its shape ([cache_size, D] under EXACT_ADAGRAD, as in the reference -- the cache rows' update is the
        row-wise one for both Adagrad kinds); a view"""
        state = self.cache_optimizer_state
        return None if state is None else state.view(-1)[:self.cache_weight.size(0)]

    def _refresh_end(self, old) -> None:
        """behind the populate: kept keys get their trained rows and state back, admitted keys start from zero state"""
        if old is not None:
            _engine.cache_carry(self.hashtbl, old[0], self.cache_state, old[1], self.cache_weight, old[2], self._cache_row_state())

    def cache_populate(self, write_back: float = 0.0, write_back_steps: int = 1, keep_trained: bool = False,
                       freq_shift: int = 0) -> None:
        """tt_embeddings_ops.py:800-814.  `write_back` (NOT in the reference; default 0 = its behaviour): cached rows are trained
        directly, and a populate decompresses every cache row anew from the cores -- what the cached copies learnt since the last
        populate is dropped.  A dense row has no exact TT representation, so there is no inverse; with write_back = lr > 0 the
        cores first take `write_back_steps` fused SGD steps of that size toward the cached rows (gradient of 1/2 ||TT row - cached row||^2
        for every cached key, through the ordinary forward / backward contraction), which moves the TT rows toward what the cache
        learnt -- an approximation (the cached keys share core slices: a few steps recover part of the difference, measured in
        tests/test_module_cpu.py), off by default.

        `keep_trained` (NOT in the reference; default False = its behaviour): a key that is cached before and
        after the populate keeps its trained row and the row's fused optimizer state, whatever row number it moves to; a key new
        to the cache gets the freshly decompressed row and zero state.  Exact, GPU only, refused together with
        reference_exact_populate; costs a transient copy of cache_weight (and state).  While the module still warms up there is
        nothing to keep.  With write_back the cores move first: kept rows keep their values, admitted rows decompress from the
        moved cores.  With sparse=False only the weights move -- an external optimizer's per-row state (momentum, Adam moments
        of cache_weight) is the caller's business.

        `freq_shift` = k in [0, 63) (NOT in the reference; default 0): cache_freq >>= k in front of the sort.  A populate zeroes
        the count of every key it evicts while cached keys keep counting from the start of the run, so without ageing the
        incumbents never leave; halving (k = 1) at every refresh makes the counts an exponential average."""
        self._refresh_check(keep_trained, freq_shift)
        if self._tables_cache():
            if write_back > 0.0:
                raise NotImplementedError("cache_populate(write_back > 0) is not supported by the row cache over several tables")
            populate = getattr(_engine, "cache_populate_tables", None)
            if populate is None or not self.cache_weight.is_cuda:
                raise NotImplementedError("the row cache over several tables is populated on the GPU only")
            extra = {"reference_exact": True} if self.reference_exact_populate else {}
            old = self._refresh_begin(keep_trained, freq_shift)
            populate(self.num_tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, list(self.tt_cores), self.hashtbl,
                     self.cache_freq, self.cache_state, self.cache_weight, self._key_stride(), **extra)
            self._refresh_end(old)
            self.warmup = False
            self._drop_prefetched()
            return
        if self.use_cache and write_back > 0.0 and not self.warmup:
            self._write_back(write_back, write_back_steps)
        if self.use_cache:
            extra = {"reference_exact": True} if self.reference_exact_populate else {}
            old = self._refresh_begin(keep_trained, freq_shift)
            _engine.cache_populate(self.num_embeddings, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks,
                                   list(self.tt_cores), self.L, self.hashtbl, self.cache_freq, self.cache_state,
                                   self.cache_weight, **extra)
            self._refresh_end(old)
            self.warmup = False
            self._drop_prefetched()  # (a planned-ahead batch was split into hits / misses by the OLD cache contents)

    def update_cache(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None) -> None:
        """count a batch in the frequency table.  Several tables: the cache counts keys table * key_stride + index, the table
        read off the batch's `offsets` (the form forward() takes), which are then required."""
        if self._tables_cache():
            if indices.numel() == 0:
                return
            if offsets is None:
                raise ValueError("update_cache(indices, offsets): the row cache over several tables needs the batch's offsets")
            indices, offsets = self._normalise(indices, offsets)
            self._count_keys(indices.contiguous(), offsets.contiguous())
            return
        if self.use_cache:
            _engine.update_cache_state(indices, self.hashtbl, self.cache_freq)

    # -------------------------------------------------------------- prefetch
    def _normalise(self, indices: torch.Tensor, offsets: torch.Tensor, closed: bool = False):
        """closed: the offsets carry their closing entry whatever include_last_offset says (the ones this module built itself)"""
        indices, offsets = indices.long(), offsets.long()
        if not self.include_last_offset and not closed:
            offsets = torch.cat([offsets, offsets.new_full((1,), indices.numel())])
        return indices, offsets

    def prefetch(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None) -> bool:
        """Not in the reference.  Run the lookup prologue of a COMING batch now, on a side stream: hash-table frequency
        update, offsets -> bag rows and the lookup plan depend on the batch's indices only, not on the cores, so they
        can overlap the backward of the step before (call it once the next batch's tensors exist, before
        `loss.backward()`; the next `forward(indices, offsets)` with the same tensor OBJECTS, unmodified, picks the
        result up -- anything else runs the prologue in line).  HIP streams
        and events only; captures into a hipGraph as a forked branch.  (Host cost of a call: ~25 us of stream / event
        handling -- worth it inside a captured step or for steps beyond ~0.1 ms; an eager loop of small steps is better served
        by prefetch_many(), one launch for a round of batches.)  Returns False (and does nothing) whenever the
        overlap does not apply: cache live, no C++ node, CPU tensors, empty batch, duplicate sharing, a module with padding_idx
        or 2-D indices (a prologue planned ahead would be over the uncompacted slots)."""
        if self.__dict__.get("padding_idx") is not None or offsets is None or indices.dim() != 1:
            return False
        if self._tables_cache():  # (the prologue planned ahead would count local indices, not keys)
            return False
        fast = _native_node()
        if (fast is None or not self.warmup or not indices.is_cuda or indices.numel() == 0 or self._dedup_may_share(indices.numel())
                or indices.dim() != 1 or offsets.dim() != 1 or self.__dict__.get("_split0", 0) > 1
                or self.__dict__.get("mode", "sum") == "max"):
            return False
        key = (id(indices), id(offsets))  # (identity: the entry keeps both objects alive, so neither id nor memory is reused)
        idx, off = self._normalise(indices, offsets)
        idx, off = idx.contiguous(), off.contiguous()
        cur = torch.cuda.current_stream(indices.device)
        side = self.prefetch_stream(indices.device)
        ready = torch.cuda.Event()
        ready.record(cur)  # the batch's tensors exist at this point of the caller's stream
        if side != cur:  # made (perhaps cast / concatenated) on the caller's stream, read on the side stream
            idx.record_stream(side)
            off.record_stream(side)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            rowidx, tableidx, plan = fast.prologue(idx, off, self.num_tables, getattr(self, "_p_flat", self.tt_p_shapes),
                                                   self.tt_q_shapes, self.tt_ranks,
                                                   self.hashtbl if self.use_cache else None,
                                                   self.cache_freq if self.use_cache else None)
            done = torch.cuda.Event()
            done.record(side)
        if len(self._prefetched) >= 8:  # (batches that never came: drop the oldest)
            self._evict_oldest_prefetched()
        self._prefetched[key] = (idx, off, (rowidx, tableidx, plan), done, indices, offsets, indices._version,
                                 offsets._version, False)
        return True

    def prefetch_many(self, batches) -> bool:
        """Not in the reference.  The lookup prologues of SEVERAL coming batches -- `[(indices, offsets), ...]`, all of
        one size -- in one launch on the current stream (`ttx_lookup_prologue_multi`): a prologue occupies 30 of the chip's
        256 CUs for its ~12 us of dependent loads, sixteen of them take about as long as one.  Each batch's next
        `forward(indices, offsets)` picks its result up, as after prefetch().  With a LIVE cache (one table) the round's
        frequency updates, cache lookups, hit / miss partitions and miss plans are done the same way
        (`ttx_lookup_prologue_cached_multi`, three launches); cache_populate() / reset_cache() drop what was planned.
        Returns False (and does nothing) where the prologue cannot be planned ahead: no C++ node, CPU tensors, empty
        batches, batches of different sizes, duplicate sharing, a live cache over several tables, a module with padding_idx, 2-D
        indices."""
        fast = _native_node()
        batches = list(batches)
        if self.__dict__.get("padding_idx") is not None or any(o is None or i.dim() != 1 for i, o in batches):
            return False
        if self._tables_cache():  # (the prologues planned ahead would count local indices, not keys)
            return False
        live = not self.warmup
        if (fast is None or not batches or self.__dict__.get("_split0", 0) > 1 or self._dedup_may_share(batches[0][0].numel())
                or (live and not (self.use_cache and self.num_tables == 1)) or self.__dict__.get("mode", "sum") == "max"):
            return False
        norm, keys = [], []
        for indices, offsets in batches:
            if not indices.is_cuda or indices.numel() == 0 or indices.dim() != 1 or offsets.dim() != 1:
                return False
            keys.append((id(indices), id(offsets)))
            idx, off = self._normalise(indices, offsets)
            norm.append((idx.contiguous(), off.contiguous()))
        if len({(i.numel(), o.numel()) for i, o in norm}) != 1:
            return False
        self.prefetch_stream(norm[0][0].device)
        if live:
            res = fast.prologue_cached_multi([i for i, _ in norm], [o for _, o in norm], self.tt_p_shapes, self.tt_q_shapes,
                                             self.tt_ranks, self.hashtbl, self.cache_freq, self.cache_state)
        else:
            res = fast.prologue_multi([i for i, _ in norm], [o for _, o in norm], self.num_tables,
                                      getattr(self, "_p_flat", self.tt_p_shapes), self.tt_q_shapes, self.tt_ranks,
                                      self.hashtbl if self.use_cache else None,
                                      self.cache_freq if self.use_cache else None)
        for k, key in enumerate(keys):
            while len(self._prefetched) >= 64:
                self._evict_oldest_prefetched()
            self._prefetched[key] = (norm[k][0], norm[k][1], tuple(t[k] for t in res), None, batches[k][0], batches[k][1],
                                     batches[k][0]._version, batches[k][1]._version, live)
        return True

    def _cached_args_stale(self, cores, state, buffers) -> bool:
        """the cached argument lists (_fa / _fc) hold the Parameter / buffer OBJECTS; anything that re-binds one --
        load_state_dict(assign=True), m.tt_cores[i] = nn.Parameter(..), register_buffer over an old name -- must not leave the
        native node training the orphaned tensors.  Identity checks against the module's own dicts: no attribute protocol, ~1 us."""
        mods = self._modules  # (the sub-modules' own dicts, reached without nn.Module.__getattr__)
        pc, ps = mods["tt_cores"]._parameters, mods["optimizer_state"]._buffers  # (BufferList: registered buffers, in order)
        if len(pc) != len(cores) or not all(map(_is, cores, pc.values())):
            return True
        if len(ps) != len(state) or not all(map(_is, state, ps.values())):
            return True
        bufs = self._buffers
        return any(t is not None and bufs.get(name) is not t for name, t in buffers)

    def _apply(self, fn, *a, **kw):
        """module.to() / .cuda() / .float(): buffers are replaced by new tensors -- forget the cached argument lists"""
        self.__dict__.pop("_fa", None)
        self.__dict__.pop("_fc", None)
        self.__dict__.pop("_sh0", None)  # (the padded copy of core 0 belongs to the old tensors' device / dtype)
        self.__dict__.pop("_fixed_off", None)
        return super()._apply(fn, *a, **kw)

    def _evict_oldest_prefetched(self) -> None:
        """drop the oldest planned-ahead batch; its frequency update has been issued, so should the batch come after
        all, its in-line prologue must not count it again (forward looks it up in _pf_evicted)"""
        k = next(iter(self._prefetched))
        hit = self._prefetched.pop(k)
        if self.use_cache:
            ev = self.__dict__.setdefault("_pf_evicted", {})
            while len(ev) >= 64:
                ev.pop(next(iter(ev)))
            ev[k] = (hit[4], hit[5], hit[6], hit[7])

    def _drop_prefetched(self, counted: bool = True) -> None:
        """forget what was planned ahead.  counted: the dropped batches' frequency updates stay in the table
        (cache_populate), so their in-line prologues must not repeat them."""
        while counted and getattr(self, "_prefetched", None):
            self._evict_oldest_prefetched()
        if getattr(self, "_prefetched", None):
            self._prefetched.clear()
        if not counted and getattr(self, "_pf_evicted", None):
            self._pf_evicted.clear()

    def __getstate__(self):
        """copy.deepcopy / torch.save of the module: the prefetch side stream and the planned-ahead batches (device
        buffers, HIP events) belong to this process and this point in time -- they are recreated at first use."""
        state = self.__dict__.copy()
        for k in ("_pf_stream", "_prefetched", "_pf_key", "_pf_counted", "_pf_evicted", "_fa", "_fc", "_fixed_off"):
            state.pop(k, None)
        return state

    def prefetch_stream(self, device: Optional[torch.device] = None) -> "torch.cuda.Stream":
        """the side stream of prefetch() (created at first use; call this before a hipGraph capture that prefetches)"""
        side = getattr(self, "_pf_stream", None)
        if side is None:
            side = self._pf_stream = torch.cuda.Stream(device=device if device is not None else self.tt_cores[0].device)
            self._prefetched = {}
        return side

    def _take_prefetched(self, indices: torch.Tensor, offsets: torch.Tensor, live: bool = False):
        """the planned-ahead prologue of this batch -- (rowidx, tableidx, plan), or with a live cache (tableidx, pcol, prow,
        ploc, n_tt, plan) -- or None"""
        d = self.__dict__  # (plain attributes, read and written past nn.Module's attribute protocol: ~1 us apiece on the host-bound step)
        pf = d.get("_prefetched")
        if not pf:
            return None
        hit = pf.pop(d.get("_pf_key"), None)
        d["_pf_key"] = None
        if hit is None:
            return None
        if hit[8] != live:  # planned for the other state of the cache: the prologue runs in line -- without counting
            d["_pf_counted"] = self.use_cache  # the batch into the frequency table a second time
            return None
        pre, done = hit[2], hit[3]
        if done is not None:  # (prefetch(): ran on the side stream; prefetch_many(): same stream, stream-ordered)
            cur = torch.cuda.current_stream(indices.device)
            cur.wait_event(done)
            for t in pre:  # allocated on the side stream, used (and freed) on this one
                t.record_stream(cur)
        return pre

    # --------------------------------------------------------------- forward
    def _forward_split0(self, fast, indices: torch.Tensor, offsets: torch.Tensor, k: int) -> torch.Tensor:
        """q0 = k q0': k part lookups per index through the C++ node on the table [k p0, p1, p2] x [q0', q1, q2] (views of
        core 0 and its optimizer state: the same memory); the output [tables, k B, D / k] IS [tables, B, D]."""
        sparse, tt_cores = self._route_args()
        use_state, optim = _optim_code(sparse, self.optimizer)
        if self.use_cache and self.num_tables == 1:  # (the frequency table counts the caller's indices, not the part lookups;
            _engine.update_cache_state(indices, self.hashtbl, self.cache_freq)  # several tables: _forward_sum counted their keys)
        p, q, nt = self.tt_p_shapes, self.tt_q_shapes, self.num_tables
        vi, vo = _engine.split0_expand(indices, offsets, k, p[1] * p[2])
        Q = self.__dict__.get("_pad0", 0) or q[0]
        c0 = tt_cores[0]
        s0 = self.optimizer_state[0] if use_state else None
        if Q != q[0]:  # core 0 (and its optimizer state) zero-padded to Q slots: `_pad0_target`
            c0, s0 = self._padded0(Q, optim, use_state, c0)
        cores = [c0.view(nt, k * p[0], c0.size(2) // k), tt_cores[1], tt_cores[2]]
        state = [s0.view(nt, k * p[0], s0.size(2) // k), self.optimizer_state[1], self.optimizer_state[2]] if use_state else []
        out = fast.lookup(vi, vo, nt, [k * p[0], p[1], p[2]], [Q // k, q[1], q[2]], self.tt_ranks, optim,
                          self.learning_rate, self.eps, None, None, state, cores, None, None, None, None)
        B = (offsets.numel() - 1) // nt
        if Q == q[0]:
            return out.view(nt, B, self.embedding_dim)
        if optim != 2 and out.grad_fn is not None:
            # the fused optimizer has updated the padded copies when this node's backward returns: the real slots go back
            # into the module's own core 0 / state 0 (what state_dict(), full_weight() and every other route read)
            out.grad_fn.register_hook(lambda gi, go: self._padded0_store())
        # (a copy, not the strided prefix view: callers of the reference's module get a contiguous [tables, B, D])
        return out.view(nt, B, Q * q[1] * q[2])[:, :, :self.embedding_dim].contiguous()

    def _padded0(self, Q: int, optim: int, use_state: bool, c0: Optional[torch.Tensor] = None):
        """core 0 [tables, p0, q0 r1] zero-padded to [tables, p0, Q r1] (and the same of its optimizer state).  Dense gradients
        (sparse=False): an autograd pad of the Parameter, every step.  Fused optimizers: a buffer the module keeps, refreshed from
        the Parameter (and the optimizer state) EVERY step -- p0 q0 r1 floats, one small copy.  (Round 4 refreshed only when the
        Parameter's `_version` moved or it was re-bound; writes through `.data` -- p.data.mul_(..), EMA / averaging code -- do not
        move the version, the next step then trained the stale copy and the write-back hook overwrote the caller's update: round 4
        advisor.)"""
        c, w = self.tt_cores[0], (Q - self.tt_q_shapes[0]) * self.tt_ranks[1]
        if optim == 2:  # (c0: core 0 as the route sees it -- `_route_args`)
            return torch.nn.functional.pad(c if c0 is None else c0, (0, w)), None
        sh = self.__dict__.get("_sh0")
        if sh is None or sh[0].device != c.device:
            mk = lambda: torch.zeros(c.size(0), c.size(1), c.size(2) + w, device=c.device, dtype=c.dtype)  # noqa: E731
            sh = self._sh0 = [mk().requires_grad_(True), mk() if use_state else None, None, -1, None, -1]
        srcs = [(0, c, 2)] + ([(1, self.optimizer_state[0], 4)] if use_state else [])
        with torch.no_grad():
            for j, src, at in srcs:
                if sh[j] is None:
                    sh[j] = torch.zeros_like(sh[0])
                sh[j][:, :, :src.size(2)].copy_(src)  # (the padded slots stay zero: nothing ever writes a non-zero there)
                sh[at], sh[at + 1] = src, src._version
        return sh[0], sh[1]

    @torch.no_grad()
    def _padded0_store(self) -> None:
        sh = self._sh0
        for j, at in ((0, 2), (1, 4)):
            src = sh[at]
            if src is not None and sh[j] is not None:
                src.copy_(sh[j][:, :, :src.size(2)])
                sh[at + 1] = src._version

    def _forward_n(self, indices: torch.Tensor, offsets: torch.Tensor, n_dev: torch.Tensor) -> torch.Tensor:
        """forward with a device-side lookup count (see forward): the prologue is built for the live lookups (C++ node:
        prologue(n_dev=) -> lookup(pre_*=)); routes that cannot take a device count read it back and slice."""
        fast = _native_node()
        plain = (fast is not None and self.warmup and indices.is_cuda and indices.numel() > 0 and not self.use_cache
                 and self.__dict__.get("_split0", 0) <= 1 and not self._dedup_may_share(indices.numel()))
        if not plain:  # (CPU tensors under the tests' oracle engine, a cache, part lookups, shared duplicates)
            if indices.is_cuda and torch.cuda.is_current_stream_capturing():
                # (round 6, advisor: this route reads the count back -- say so instead of failing inside the capture)
                raise RuntimeError("TableBatchedTTEmbeddingBag.forward(n_dev=): with a cache, part lookups (q0 > 4) or shared duplicates "
                                   "the live count is read back to the host -- not capturable in a hipGraph on this route")
            n = int(n_dev.item())
            return self._forward_sum(indices[:n].contiguous(), offsets, closed=True)  # (n_dev: offsets with their closing entry)
        indices = indices.long() if indices.dtype != torch.int64 else indices
        offsets = offsets.long() if offsets.dtype != torch.int64 else offsets
        indices = indices if indices.is_contiguous() else indices.contiguous()
        offsets = offsets if offsets.is_contiguous() else offsets.contiguous()
        sparse, tt_cores = self._route_args()
        use_state, optim = _optim_code(sparse, self.optimizer)
        p_flat = getattr(self, "_p_flat", self.tt_p_shapes)
        pre = fast.prologue(indices, offsets, self.num_tables, p_flat, self.tt_q_shapes, self.tt_ranks, None, None,
                            n_dev.to(torch.int32).reshape(1))
        return fast.lookup(indices, offsets, self.num_tables, p_flat, self.tt_q_shapes, self.tt_ranks, optim,
                           self.learning_rate, self.eps, None, None, list(self.optimizer_state) if use_state else [],
                           list(tt_cores), None, *pre)

    def _det_bits(self) -> int:
        """the C++ node's encoding of deterministic_cache_update (csrc/ttx_torch.cpp: bit 9 sorted, bit 10 atomics, neither auto)"""
        det = self.__dict__.get("deterministic_cache_update")
        if det is None and os.environ.get("TTX_DETERMINISTIC", "") != "":
            det = os.environ["TTX_DETERMINISTIC"] not in ("0", "")
        return 0 if det is None else (512 if det else 1024)

    def _dedup_may_share(self, nnz: int) -> bool:
        d = getattr(self, "dedup", False)
        return bool(d) and (d != "auto" or nnz >= _DEDUP_AUTO_MIN_NNZ)

    def _dedup_auto(self, nnz: int):
        """dedup="auto": (share this batch?, sample its distinct fraction?)."""
        if nnz < _DEDUP_AUTO_MIN_NNZ:
            return False, False
        st = self.__dict__.setdefault("_dd_auto", [False, 0])
        if st[1] <= 0 and not torch.cuda.is_current_stream_capturing():
            return True, True
        st[1] -= 1
        return st[0], False

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None, warmup: bool = True,
                per_sample_weights: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """-> [num_tables, B, D].  (`warmup` is ignored like in the reference,
        which uses self.warmup, :822,:841.)  int32 indices / offsets are accepted; with
        include_last_offset=False the closing offset (nnz) is appended here.
        `n_dev` (round 5; not in the reference): one int32 on the device, the number of LIVE lookups -- `indices` then holds an
        upper bound (a fixed-capacity buffer), `offsets` (with its closing entry) describes exactly the first n_dev of them, and
        only those are planned, contracted, pooled and trained: no host read-back of the count (ttx_lookup_prologue_n).  What
        the table-sharded module's ragged route hands its local lookup.
        The bags are pooled by the constructor's `mode` ("sum": the reference's).
        nn.EmbeddingBag's padded batches: `indices` [N, L] with `offsets=None` is N = num_tables * B bags of L slots each
        (table-major, `per_sample_weights` then [N, L] too), and with the constructor's `padding_idx` the slots that hold it are
        dropped in front of the lookup (`_forward_padded`)."""
        d = self.__dict__
        if offsets is None or indices.dim() != 1 or d.get("padding_idx") is not None:
            return self._forward_padded(indices, offsets, warmup, per_sample_weights, n_dev)
        if d.get("mode", "sum") != "sum":
            return self._forward_mode(indices, offsets, warmup, per_sample_weights, n_dev)
        return self._forward_sum(indices, offsets, warmup, per_sample_weights, n_dev)

    def _fixed_offsets(self, device: torch.device, N: int, L: int) -> torch.Tensor:
        """arange(0, N L + 1, L): the offsets (closing entry included) of N bags of L slots, kept per (device, N, L)"""
        cache = self.__dict__.setdefault("_fixed_off", {})
        key = (device, N, L)
        off = cache.get(key)
        if off is None:
            while len(cache) >= 8:
                cache.pop(next(iter(cache)))
            off = torch.arange(0, N * L + 1, L, dtype=torch.int64, device=device) if L > 0 \
                else torch.zeros(N + 1, dtype=torch.int64, device=device)
            cache[key] = off
        return off

    def _forward_closed(self, indices, offsets, warmup, per_sample_weights) -> torch.Tensor:
        """the existing routes on offsets that carry their closing entry"""
        if self.__dict__.get("mode", "sum") != "sum":
            return self._forward_mode(indices, offsets, warmup, per_sample_weights, None, closed=True)
        return self._forward_sum(indices, offsets, warmup, per_sample_weights, None, closed=True)

    def _forward_padded(self, indices, offsets, warmup, per_sample_weights, n_dev) -> torch.Tensor:
        """nn.EmbeddingBag's 2-D fixed-length input and padding_idx.  Without padding_idx the 2-D input is
        the flattened batch with offsets 0, L, 2L, ...; with it the padding slots are dropped in front of the lookup: on the
        device by `bags_compact` + the n_dev route (sum / mean: no host read-back, capturable where forward(n_dev=) is), with a
        read-back of the live count for max (forward(n_dev=) is not offered there), with torch ops where per_sample_weights must
        keep their autograd path or the tensors are on the CPU."""
        pad = self.__dict__.get("padding_idx")
        mode = self.__dict__.get("mode", "sum")
        if n_dev is not None:
            raise NotImplementedError("forward(n_dev=) takes a compacted 1-D batch: not 2-D indices, not a module with padding_idx")
        if indices.dim() == 2:
            if offsets is not None:
                raise ValueError("if indices is 2-D, offsets has to be None: indices is a batch of fixed-length bags (as in torch)")
            N, L = int(indices.size(0)), int(indices.size(1))
        elif indices.dim() == 1:
            if offsets is None:
                raise ValueError("offsets has to be a 1-D tensor when indices is 1-D (as in torch)")
            if offsets.dim() != 1:
                raise ValueError("offsets must be 1-D")
            L = 0
        else:
            raise ValueError(f"indices must be 1-D or 2-D, got {indices.dim()}-D")
        if per_sample_weights is not None:
            if mode != "sum":
                raise ValueError(f"per_sample_weights is only supported with mode='sum' (as in torch), not mode={mode!r}")
            if per_sample_weights.shape != indices.shape:
                raise ValueError("per_sample_weights must have the shape of indices")
            per_sample_weights = per_sample_weights.reshape(-1)
        if offsets is None:  # N bags of L slots; with padding on the device the kernel takes L itself
            indices = indices.reshape(-1)
            if pad is None or L == 0 or per_sample_weights is not None or not indices.is_cuda:
                offsets = self._fixed_offsets(indices.device, N, L)
        else:
            indices, offsets = self._normalise(indices, offsets)
            N = offsets.numel() - 1
        if N % self.num_tables != 0:
            raise ValueError(f"the batch must hold num_tables * B bags, got {N} bags for {self.num_tables} tables")
        if pad is None:
            return self._forward_closed(indices, offsets, warmup, per_sample_weights)
        if per_sample_weights is not None or not indices.is_cuda:
            # torch ops: boolean indexing keeps the weights' autograd path (padding slots get a zero weight gradient) -- and is what
            # the tests' CPU engine runs.  The number of live slots shapes the result: a host synchronisation.
            if indices.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("padding_idx with per_sample_weights drops the padding with torch ops, whose output shape is the "
                                   "live count read back to the host -- not capturable in a hipGraph")
            keep = indices != pad
            before = torch.cat([torch.zeros(1, dtype=torch.int64, device=indices.device), torch.cumsum(keep, 0)])
            offsets = before[offsets.long().clamp(0, indices.numel())]  # live slots in front of every bag start
            if per_sample_weights is not None:
                per_sample_weights = per_sample_weights[keep]
            return self._forward_closed(indices[keep], offsets, warmup, per_sample_weights)
        if mode == "max" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("padding_idx with mode='max' reads the live count back to the host (forward(n_dev=) is not "
                               "offered for max) -- not capturable in a hipGraph")
        indices = indices.long() if indices.dtype != torch.int64 else indices
        live, bag_offsets, n_live = _engine.bags_compact(indices.contiguous(), offsets, L, pad)
        if mode == "max":
            return self._forward_closed(live[:int(n_live.item())], bag_offsets, warmup, None)
        summed = self._forward_n(live, bag_offsets, n_live)
        return summed if mode == "sum" else TTMeanPoolFunction.apply(summed, bag_offsets)

    def _forward_mode(self, indices, offsets, warmup, per_sample_weights, n_dev, closed: bool = False) -> torch.Tensor:
        """mode="mean": the sum lookup (any route) scaled per bag; mode="max": TTMaxLookupFunction on the unsplit geometry."""
        if per_sample_weights is not None:
            raise ValueError(f"per_sample_weights is only supported with mode='sum' (as in torch), not mode={self.mode!r}")
        if self.mode == "max":
            if n_dev is not None:
                raise NotImplementedError("mode='max' does not support forward(n_dev=)")
            if indices.dim() != 1 or offsets.dim() != 1:
                raise ValueError("indices and offsets must be 1-D (the 2-D fixed-length form of nn.EmbeddingBag is not supported)")
            indices, offsets = self._normalise(indices, offsets, closed)
            if (offsets.numel() - 1) % self.num_tables != 0:
                raise ValueError(f"offsets must describe num_tables * B bags, got {offsets.numel() - 1} bags for "
                                 f"{self.num_tables} tables")
            # (q0 > 4: the unsplit geometry on the generic kernels -- the part lookups of the sum route would split a bag's
            #  columns over k part bags, each with its own winner per column, which is the same max, but their gradient rows
            #  would need the part layout: not worth a route of its own)
            sparse, tt_cores = self._route_args(indices.numel() > 0)
            return TTMaxLookupFunction.apply(
                (offsets.numel() - 1) // self.num_tables, self.embedding_dim, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks,
                indices.contiguous(), offsets.contiguous(), self.optimizer, self.learning_rate, self.eps, sparse,
                list(self.optimizer_state), *tt_cores)
        # mean: the bag lengths come from the offsets in their closing-entry form (n_dev: the caller's, which must have it)
        bag_offsets = offsets.long() if n_dev is not None else self._normalise(indices, offsets, closed)[1]
        summed = self._forward_sum(indices, offsets, warmup, None, n_dev, closed)
        return TTMeanPoolFunction.apply(summed, bag_offsets.contiguous())

    def _forward_sum(self, indices: torch.Tensor, offsets: torch.Tensor, warmup: bool = True,
                     per_sample_weights: Optional[torch.Tensor] = None, n_dev: Optional[torch.Tensor] = None,
                     closed: bool = False) -> torch.Tensor:
        if n_dev is not None:
            if per_sample_weights is not None:  # (round 6, advisor: the weights were silently dropped on this route)
                raise NotImplementedError("forward(n_dev=) does not take per_sample_weights")
            if not self.include_last_offset:
                raise ValueError("forward(n_dev=) needs offsets with their closing entry (include_last_offset=True): the closing "
                                 "offset IS the live count, which only the device knows")
            return self._forward_n(indices, offsets, n_dev)
        if per_sample_weights is not None:
            # nn.EmbeddingBag(mode="sum") semantics: forward, the cores' gradients / fused optimizers and -- if the
            # weights require it -- their own gradient.  Served by the C++ nodes: cache not live, or live over one table
            # (the weights follow their lookups through the hit / miss partition; cache rows are gathered and updated
            # weighted).
            if _native_node() is None or not indices.is_cuda or (not self.warmup and not (self.use_cache and self.num_tables == 1)):
                raise NotImplementedError("per_sample_weights needs ttx_torch.so (GPU tensors)")
            if per_sample_weights.shape != indices.shape:
                raise ValueError("per_sample_weights must have the shape of indices")
            per_sample_weights = per_sample_weights.float().contiguous()  # (keeps the autograd graph of the weights)
        if indices.dim() != 1 or offsets.dim() != 1:
            raise ValueError("indices and offsets must be 1-D (the 2-D fixed-length form of nn.EmbeddingBag is not supported)")
        d = self.__dict__  # (plain attributes past nn.Module's __setattr__ / __getattr__: 1.3 / 0.8 us apiece, five per call)
        d["_pf_key"] = None
        d["_pf_counted"] = False  # this batch's frequency update was issued by a planned-ahead prologue that is not used
        if d.get("_prefetched"):  # a prefetch() for exactly these tensor objects, not written to since?
            k = (id(indices), id(offsets))
            hit = self._prefetched.get(k)
            if hit is not None and (hit[4] is not indices or hit[5] is not offsets or hit[6] != indices._version
                                    or hit[7] != offsets._version):
                self._prefetched.pop(k)  # stale: the batch was modified in place after its prefetch
                hit = None
            if hit is not None:
                d["_pf_key"] = k
                indices, offsets = hit[0], hit[1]  # (already in the int64 / closing-offset form)
        if self._pf_key is None:
            ev = d.get("_pf_evicted")
            if ev:
                e = ev.pop((id(indices), id(offsets)), None)
                if e is not None and e[0] is indices and e[1] is offsets and e[2] == indices._version and e[3] == offsets._version:
                    d["_pf_counted"] = True
            indices, offsets = self._normalise(indices, offsets, closed)
        if (offsets.numel() - 1) % self.num_tables != 0:
            raise ValueError(f"offsets must describe num_tables * B bags, got {offsets.numel() - 1} bags for "
                             f"{self.num_tables} tables")
        fast = _native_node()
        count_local = d["use_cache"]  # the route's own frequency update counts the indices as they are (one table)
        if count_local and (d["num_tables"] > 1 or self._tables_cache()):
            # ONE row cache over all tables: the frequency table holds keys table * key_stride + index
            # (tables of different row factors, DESIGN.md 4.14: key_base[table] + index -- `_key_space`)
            count_local = False
            if not self.warmup and indices.numel() > 0:
                if not indices.is_cuda or getattr(_engine, "table_keys", None) is None:
                    raise NotImplementedError("a live row cache over several tables serves GPU tensors only")
                if per_sample_weights is not None:
                    raise NotImplementedError("per_sample_weights with a live row cache over several tables")
                use_state, _ = _optim_code(self.sparse, self.optimizer)
                return TTTablesCachedLookupFunction.apply(
                    (offsets.numel() - 1) // self.num_tables, self.embedding_dim, self.num_tables, self._key_space(),
                    self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, self.L, indices.contiguous(), offsets.contiguous(),
                    self.hashtbl, self.cache_state, self.cache_freq, d.get("deterministic_cache_update"), self.optimizer,
                    self.learning_rate, self.eps, self.sparse, self.cache_optimizer_state if use_state else None,
                    self.cache_weight, list(self.optimizer_state), *self.tt_cores)
            if self.warmup:
                # warm-up: the batch's keys are counted here (one extra launch), and the lookup runs on the existing routes
                # with their own frequency update switched off
                self._count_keys(indices.contiguous(), offsets.contiguous())
                d["_pf_counted"] = True
        share = getattr(self, "dedup", False) and self.warmup and indices.is_cuda and indices.numel() > 0 \
            and per_sample_weights is None and getattr(_engine, "DedupPlan", None) is not None
        sample = False
        if share and self.dedup == "auto":
            share, sample = self._dedup_auto(indices.numel())
        if share:
            # duplicate lookups share their contraction: frequency update + bag rows as usual, then the map and the
            # plan of the distinct pairs (one work-group sorts the batch's keys), through the reference-shaped route
            indices, rowidx, tableidx, n_tt, cache_locations = _engine.preprocess_indices_sync(
                indices, offsets, self.num_tables, True, self.hashtbl, self.cache_state,
                *((self.cache_freq,) if count_local else ()))
            rowidx._ttx_plan = _engine.make_plan(self.num_tables, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks,
                                                 n_tt, indices, tableidx, rowidx, dedup=True)
            if sample:  # the map's header holds the number of distinct pairs (one read-back per sampling period)
                dd = getattr(rowidx._ttx_plan, "dd", None)
                frac = float(dd[:4].view(torch.int32).item()) / max(n_tt, 1) if dd is not None else 1.0
                self._dd_auto = [frac <= _DEDUP_AUTO_MAX_DISTINCT, _DEDUP_AUTO_PERIOD]
                self._dd_auto_last = frac
            sparse, tt_cores = self._route_args()
            return TTLookupFunction.apply(
                (offsets.numel() - 1) // self.num_tables, self.embedding_dim, self.tt_p_shapes, self.tt_q_shapes,
                self.tt_ranks, self.L, n_tt, 0, indices, rowidx, tableidx, self.optimizer, self.learning_rate,
                self.eps, sparse, None, self.cache_optimizer_state, self.cache_weight,
                list(self.optimizer_state), *tt_cores)
        if (self.__dict__.get("_split0", 0) > 1 and fast is not None and self.warmup and indices.is_cuda and indices.numel() > 0
                and per_sample_weights is None and not hasattr(self, "_p_flat")):
            return self._forward_split0(fast, indices, offsets, self._split0)
        if fast is not None and self.warmup and indices.is_cuda and indices.numel() > 0:
            # cache not live: the whole lookup (prologue, forward, and the backward / fused optimizer node)
            # is the C++ autograd node of csrc/ttx_torch.cpp -- same C ABI calls, no interpreter in between
            adam = d.get("_adam") is not None  # (EXACT_ADAM: dense gradients of the cores as `_route_args` hands them on)
            use_state = self.sparse and self.optimizer not in _SGD_LIKE and not adam
            optim = 2 if not self.sparse or adam else (1 if use_state else 0)
            pre = self._take_prefetched(indices, offsets)  # (rowidx, tableidx, plan) if prefetch() ran for this batch
            count = self.use_cache and not self._pf_counted
            fa = self.__dict__.get("_fa")  # (cores, state, hashtbl, cache_freq, p): looked up once, not per step -- every
            if fa is not None and self._cached_args_stale(fa[0], fa[1], (("hashtbl", fa[2]), ("cache_freq", fa[3]))):
                fa = None                  #  (a Parameter / buffer was re-bound: load_state_dict(assign=True), tt_cores[i] = ..)
            if fa is None:                 #  nn.Module attribute / ParameterList access is microseconds of a host-bound step
                fa = self._fa = (list(self.tt_cores), list(self.optimizer_state), self.hashtbl if self.use_cache else None,
                                 self.cache_freq if self.use_cache else None,
                                 getattr(self, "_p_flat", self.tt_p_shapes))  # (per-table factors: flattened)
            if adam:  # (this step's aliases of the cores, in the place of the Parameters)
                fa = (self._route_args()[1],) + fa[1:]
            out = fast.lookup(indices if indices.is_contiguous() else indices.contiguous(),
                              offsets if offsets.is_contiguous() else offsets.contiguous(), self.num_tables, fa[4],
                              self.tt_q_shapes, self.tt_ranks, optim, self.learning_rate, self.eps,
                              fa[2] if count else None, fa[3] if count else None,
                              fa[1] if use_state else [], fa[0], per_sample_weights,
                              *(pre if pre is not None else (None, None, None)))
            if optim != 2 and _DIRECT_BACKWARD and out.requires_grad and (per_sample_weights is None or not per_sample_weights.requires_grad):
                _direct_register(out, fast.node_of(out))  # (fused optimizer: backward() of this tensor may skip autograd's engine)
            return out
        if (fast is not None and not self.warmup and self.use_cache and self.num_tables == 1 and indices.is_cuda
                and indices.numel() > 0):
            # cache live: frequency update + hash lookup + stable partition (split point kept on the device),
            # contraction of the misses, gather of the hits, and the matching backward -- the C++ node again
            use_state = self.sparse and self.optimizer not in _SGD_LIKE
            optim = 2 if not self.sparse else (1 if use_state else 0)
            pre = self._take_prefetched(indices, offsets, live=True)  # planned ahead by prefetch_many()?
            if per_sample_weights is not None and pre is not None:
                pre = None  # (the planned-ahead partition does not carry weights: this batch's prologue runs in line,
                self._pf_counted = True  # without counting the batch a second time)
            fc = self.__dict__.get("_fc")  # (the module's tensors, looked up once: see _fa above)
            if fc is not None and self._cached_args_stale(fc[0], fc[1], (("hashtbl", fc[2]), ("cache_freq", fc[3]), ("cache_state", fc[4]),
                                                                         ("cache_optimizer_state", fc[5]), ("cache_weight", fc[6]))):
                fc = None
            if fc is None:
                fc = self._fc = (list(self.tt_cores), list(self.optimizer_state), self.hashtbl, self.cache_freq, self.cache_state,
                                 self.cache_optimizer_state, self.cache_weight)
            out = fast.lookup_cached(indices if indices.is_contiguous() else indices.contiguous(),
                                     offsets if offsets.is_contiguous() else offsets.contiguous(), self.tt_p_shapes, self.tt_q_shapes,
                                     self.tt_ranks, optim | (256 if self._pf_counted else 0) | self._det_bits(), self.learning_rate, self.eps,
                                     fc[2], fc[3], fc[4], fc[5] if use_state else None,
                                     fc[6], fc[1] if use_state else [],
                                     fc[0], list(pre) if pre is not None else [], per_sample_weights)
            if optim != 2 and _DIRECT_BACKWARD and out.requires_grad and (per_sample_weights is None or not per_sample_weights.requires_grad):
                _direct_register(out, fast.node_of(out))
            return out
        prologue = getattr(_engine, "lookup_prologue", None)
        if prologue is not None and self.warmup and indices.numel() > 0:
            # cache not live: frequency update, offsets -> bag rows and the lookup plan in one native call
            rowidx, tableidx, plan = prologue(indices, offsets, self.num_tables, self.tt_p_shapes, self.tt_q_shapes,
                                              self.tt_ranks, self.hashtbl if count_local else None,
                                              self.cache_freq if count_local else None)
            rowidx._ttx_plan = plan  # picked up by TTLookupFunction.forward
            n_tt, cache_locations = indices.numel(), None
        elif count_local and getattr(_engine, "FUSED_CACHE_UPDATE", False) and indices.numel() > 0:
            # frequency update folded into the preprocessing launch (same order as the reference:
            # count the batch's indices, then look them up)
            indices, rowidx, tableidx, n_tt, cache_locations = _engine.preprocess_indices_sync(
                indices, offsets, self.num_tables, self.warmup, self.hashtbl, self.cache_state, self.cache_freq)
        else:
            if count_local:
                self.update_cache(indices)
            indices, rowidx, tableidx, n_tt, cache_locations = _engine.preprocess_indices_sync(
                indices, offsets, self.num_tables, self.warmup, self.hashtbl, self.cache_state)
        n_cached = indices.numel() - n_tt
        det = self.__dict__.get("deterministic_cache_update")
        if det is not None and n_cached > 0:
            rowidx._ttx_det = bool(det)  # (picked up by TTLookupFunction.forward, like the plan: the reference's 19 arguments stay)
        sparse, tt_cores = self._route_args(indices.numel() > 0)
        return TTLookupFunction.apply(
            (offsets.numel() - 1) // self.num_tables, self.embedding_dim, self.tt_p_shapes, self.tt_q_shapes,
            self.tt_ranks, self.L, n_tt, n_cached, indices, rowidx, tableidx, self.optimizer, self.learning_rate,
            self.eps, sparse, cache_locations, self.cache_optimizer_state, self.cache_weight,
            list(self.optimizer_state), *tt_cores)

    def set_learning_rate(self, lr: float) -> None:
        """takes effect on the next step (every fused optimizer, OptimType.EXACT_ADAM included; eager steps between graph captures
        too).  A step captured in a hipGraph has its learning rate baked in: capture again after changing it."""
        self.learning_rate = lr

    def get_params(self) -> List[torch.Tensor]:
        params = list(self.tt_cores)
        if self.use_cache:
            params.append(self.cache_weight)
        return params


class TTEmbeddingBag(TableBatchedTTEmbeddingBag):
    """TT embedding bag for exactly one table; forward returns [B, D]."""

    def __init__(self, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, use_cache: bool = True, cache_size: int = 0, hashtbl_size: int = 0,
                 weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 device: Optional[torch.device] = None, include_last_offset: bool = True, dedup: bool = False,
                 reference_exact_populate: bool = False, deterministic_cache_update: Optional[bool] = None,
                 mode: str = "sum", padding_idx: Optional[int] = None, betas: Tuple[float, float] = (0.9, 0.999),
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False) -> None:
        super().__init__(1, num_embeddings, embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, optimizer,
                         learning_rate, eps, sparse, use_cache, cache_size, hashtbl_size, weight_dist,
                         enforce_embedding_dim, device, include_last_offset, dedup, reference_exact_populate,
                         deterministic_cache_update, mode, padding_idx, betas, weight_decay, decoupled_weight_decay)

    _STACKED_TABLES = False

    @classmethod
    def _construct(cls, num_embeddings, embedding_dim: int, tt_ranks, tt_p_shapes, tt_q_shapes, kw: dict):
        if len(num_embeddings) != 1:
            raise ValueError(f"{cls.__name__} holds one table, got {len(num_embeddings)}")
        return cls(num_embeddings[0], embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, **kw)

    def forward(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None, warmup: bool = True,
                per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        # squeeze is a view both ways: `[0]` would make autograd materialise a zero [1,B,D] buffer
        # and copy the gradient into it (two extra kernels per step)
        out = super().forward(indices, offsets, warmup, per_sample_weights)
        res = out.squeeze(0)
        e = _direct.get(id(out)) if _direct else None
        if e is not None and e[0]() is out:  # (the lookup's own node: backward() of the view is backward() of the node)
            _direct_register(res, e[1])
        return res


class TTEmbedding(TTEmbeddingBag):
    """Not in the reference: the UNPOOLED lookup, `nn.Embedding` on a TT table.  `emb(indices)` takes int64 / int32 indices of
    any shape (0-D .. n-D) and returns `indices.shape + (D,)` float32 = `F.embedding(indices, W0)`, W0 = full_weight() with row
    `padding_idx` zeroed: padding positions are exact zeros, receive no gradient and cost no contraction (they are dropped on
    the device in front of the lookup and put back behind it; a TT table holds no independent padding row, see
    TTEmbeddingBag).  Gradients as in the bag modules: `sparse=True` applies the fused SGD / Adagrad inside backward,
    `sparse=False` leaves dense gradients on `tt_cores[t].grad`.  Parameters, buffers and state_dict() are those of
    `TTEmbeddingBag(use_cache=False)` of the same geometry (the default; see `use_cache` below): a checkpoint loads in either direction.

    Routes, all without a host synchronisation unless noted: plain -- a plan without bag rows, the contraction
    straight into the output buffer, the per-lookup backward; padding_idx -- bags_compact over one-slot bags, the plan of the
    device-side live count, rows_expand / rows_collect; q0 > 4 with an exact split -- the part lookups of the core-0 row split,
    a rows buffer [N, D] being the parts' [k N, D / k]; dedup=True -- the bag module's duplicate-sharing sequence with one bag per
    position (with padding_idx the live count is read back: not capturable); CPU tensors -- the bag module's reference-shaped
    route, one bag per live position (what the tests' oracle engine runs).

    `use_cache=True` (with `cache_size`, `hashtbl_size`, `reference_exact_populate`, `deterministic_cache_update` as in
    TTEmbeddingBag, whose parameters, buffers and state_dict() the module then has): the LFU row cache under the unpooled call
    form.  While the cache warms up the routes above run, the batch's live indices counted first (`dedup` applies here only);
    after cache_populate() TTRowsCachedLookupFunction takes over -- the live preprocess with its split point on the device over N
    one-slot bags (so a partitioned lookup's bag row IS its position), the plan and contraction of the misses, rows_place (the
    misses' rows and the hits' cache rows to their positions, zeros at the padding), and backward rows_pick, the per-lookup
    backward and the cache rows' update (SGD, row-wise Adagrad, or the dense gradient of cache_weight) from the split point on.
    Nothing is read back without padding_idx: the step is capturable and the hit / miss split is not baked into the graph; with
    padding_idx the live count is read back (RuntimeError under capture).  q0 > 4 with an exact split: the misses take the part
    lookups, cached rows are whole rows.
    No table batching, no prefetch, no C++ node, no max_norm / scale_grad_by_freq."""

    def __init__(self, num_embeddings: int, embedding_dim: int, tt_ranks: List[int],
                 tt_p_shapes: Optional[List[int]] = None, tt_q_shapes: Optional[List[int]] = None,
                 optimizer: OptimType = OptimType.SGD, learning_rate: float = 0.1, eps: float = 1.0e-10,
                 sparse: bool = True, weight_dist: str = "approx-normal", enforce_embedding_dim: bool = False,
                 device: Optional[torch.device] = None, padding_idx: Optional[int] = None, dedup: bool = False,
                 use_cache: bool = False, cache_size: int = 0, hashtbl_size: int = 0, reference_exact_populate: bool = False,
                 deterministic_cache_update: Optional[bool] = None, betas: Tuple[float, float] = (0.9, 0.999),
                 weight_decay: float = 0.0, decoupled_weight_decay: bool = False) -> None:
        super().__init__(num_embeddings, embedding_dim, tt_ranks, tt_p_shapes, tt_q_shapes, optimizer, learning_rate, eps,
                         sparse, use_cache=bool(use_cache), cache_size=cache_size, hashtbl_size=hashtbl_size, weight_dist=weight_dist,
                         enforce_embedding_dim=enforce_embedding_dim, device=device, include_last_offset=True, dedup=bool(dedup),
                         reference_exact_populate=reference_exact_populate, deterministic_cache_update=deterministic_cache_update,
                         mode="sum", padding_idx=padding_idx, betas=betas, weight_decay=weight_decay,
                         decoupled_weight_decay=decoupled_weight_decay)

    def _ctor_kwargs(self) -> dict:
        kw = super()._ctor_kwargs()
        for name in ("include_last_offset", "mode"):  # (not this constructor's)
            kw.pop(name)
        return kw

    def prefetch(self, indices: torch.Tensor, offsets: Optional[torch.Tensor] = None) -> bool:
        return False  # (no prologue to plan ahead: there are no bags)

    def prefetch_many(self, batches) -> bool:
        return False

    def _bag_rows(self, live: torch.Tensor) -> torch.Tensor:
        """the bag module's sum route with one bag per lookup -> [n, D] (CPU tensors, duplicate sharing)"""
        n = live.numel()
        return self._forward_sum(live, self._fixed_offsets(live.device, n, 1), closed=True).view(n, self.embedding_dim)

    def _split_geometry(self, use_state: bool, tt_cores=None):
        """-> (k, p, q, cores, state): the geometry a rows lookup runs on.  q0 = k q0' with an exact split: k part lookups per
        position in the table [k p0, p1, p2] x [q0', q1, q2] (views of core 0 and its optimizer state: the same memory); k = 1
        otherwise (the module's own geometry)."""
        k = self.__dict__.get("_split0", 0) if not self.__dict__.get("_pad0", 0) else 0
        k = k if k > 1 else 1
        p, q = self.tt_p_shapes, self.tt_q_shapes
        cores, state = list(self.tt_cores if tt_cores is None else tt_cores), list(self.optimizer_state) if use_state else []
        if k > 1:
            c0 = cores[0]
            cores[0] = c0.view(1, k * p[0], c0.size(2) // k)
            if use_state:
                state[0] = state[0].view(1, k * p[0], state[0].size(2) // k)
            p, q = [k * p[0], p[1], p[2]], [q[0] // k, q[1], q[2]]
        return k, p, q, cores, state

    def _no_live_rows(self, flat: torch.Tensor, N: int) -> torch.Tensor:
        """no live lookup (an empty batch, or N positions of padding only) -> [N, D] zeros through the empty lookup's node, whose
        backward trains nothing and gives zero dense gradients"""
        sparse, tt_cores = self._route_args(False)
        out = TTRowsLookupFunction.apply(0, self.embedding_dim, 1, self.tt_p_shapes, self.tt_q_shapes, self.tt_ranks, flat[:0], None,
                                         None, self.optimizer, self.learning_rate, self.eps, sparse,
                                         list(self.optimizer_state), *tt_cores)
        return out if N == 0 else torch.zeros((N, self.embedding_dim), dtype=torch.float32, device=flat.device) + out.sum()

    def _forward_cached(self, flat: torch.Tensor, N: int, pad: Optional[int], use_state: bool) -> torch.Tensor:
        """GPU tensors, the cache live -> [N, D] (TTRowsCachedLookupFunction).  Without padding_idx nothing is read back; with it
        the live count is (it sizes the partition), as in the bag module."""
        D, dev = self.embedding_dim, flat.device
        rank, n = None, N
        if pad is not None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TTEmbedding(use_cache=True, padding_idx=): with a live cache the live count is read back to the "
                                   "host to size the hit / miss partition -- not capturable in a hipGraph on this route")
            flat, rank, n_live = _engine.bags_compact(flat, None, 1, pad)
            n = int(n_live.item())
            if n == 0:  # padding only: zeros, nothing trained, nothing counted (zero dense gradients, as an empty batch gives)
                return self._no_live_rows(flat, N)
            flat = flat[:n]
        k, p, q, cores, state = self._split_geometry(use_state)
        unit = self._fixed_offsets(dev, n, 1)
        return TTRowsCachedLookupFunction.apply(
            N, D, k, p, q, self.tt_ranks, flat, unit if rank is None else rank, rank, unit if k > 1 else None, self.hashtbl,
            self.cache_state, self.cache_freq, self.__dict__.get("deterministic_cache_update"), self.optimizer, self.learning_rate,
            self.eps, self.sparse, self.cache_optimizer_state if use_state else None, self.cache_weight, state, *cores)

    def forward(self, indices: torch.Tensor) -> torch.Tensor:  # noqa: D102 -- see the class
        if indices.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"indices must be int64 or int32, got {indices.dtype}")
        shape, D = tuple(indices.shape), self.embedding_dim
        flat = indices.reshape(-1)
        flat = flat.long() if flat.dtype != torch.int64 else flat
        flat = flat if flat.is_contiguous() else flat.contiguous()
        N = flat.numel()
        pad = self.__dict__.get("padding_idx")
        use_state, _ = _optim_code(self.sparse and self.__dict__.get("_adam") is None, self.optimizer)
        if N == 0:
            return self._no_live_rows(flat, 0).view(shape + (D,))
        if not flat.is_cuda:
            # the tests' oracle engine: the bag module's reference-shaped route with one bag per live position, the padding
            # dropped (and the rows put back) with torch ops
            if pad is None:
                return self._bag_rows(flat).view(shape + (D,))
            keep = torch.nonzero(flat != pad).flatten()
            out = torch.zeros((N, D), dtype=torch.float32, device=flat.device)
            if keep.numel() == 0:  # (zero dense gradients, as an empty batch gives; EXACT_ADAM: no step)
                out = out + sum(c.sum() for c in self._route_args(False)[1]) * 0.0
            else:
                out = out.index_put((keep,), self._bag_rows(flat[keep].contiguous()))
            return out.view(shape + (D,))
        if self.use_cache and not self.warmup:
            return self._forward_cached(flat, N, pad, use_state).view(shape + (D,))
        if self.dedup:
            # duplicate positions share one contraction: the bag module's sequence (make_plan(dedup=True), ttx_tt_forward_dd /
            # _backward_dd) with B = N bags of one lookup; a batch ttx_dedup_bytes refuses takes the plain plan there
            # (while a cache warms up that sequence counts the batch's live indices itself)
            if pad is None:
                return self._bag_rows(flat).view(shape + (D,))
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("TTEmbedding(dedup=True, padding_idx=): the live count is read back to the host to size the "
                                   "duplicate map -- not capturable in a hipGraph on this route")
            live, rank, n_live = _engine.bags_compact(flat, None, 1, pad)
            n = int(n_live.item())
            if n == 0:
                return self._no_live_rows(flat, N).view(shape + (D,))
            return _RowsAtPositionsFunction.apply(self._bag_rows(live[:n].contiguous()), rank).view(shape + (D,))
        rank = n_dev = None
        if pad is not None:
            flat, rank, n_dev = _engine.bags_compact(flat, None, 1, pad)
        if self.use_cache:
            # the cache warms up: the existing routes, the batch's LIVE indices counted first (with padding_idx the live count
            # is read back for that, as the bag module does for a cache beside padding)
            if pad is None:
                self.update_cache(flat)
            else:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("TTEmbedding(use_cache=True, padding_idx=): the live count is read back to the host to count "
                                       "the live indices -- not capturable in a hipGraph on this route")
                self.update_cache(flat[:int(n_dev.item())])
        sparse, tt_cores = self._route_args()
        k, p, q, cores, state = self._split_geometry(use_state, tt_cores)
        if k > 1:
            # position n's parts are lookups k n .. k n + k - 1, their rows of D / k columns ARE row n of [N, D]; of a compacted
            # batch the first k n_live part lookups are the live ones
            flat, _ = _engine.split0_expand(flat, self._fixed_offsets(flat.device, N, 1), k, p[1] * p[2])
            if n_dev is not None:
                n_dev = n_dev * k
        out = TTRowsLookupFunction.apply(N, D, k, p, q, self.tt_ranks, flat, rank, n_dev, self.optimizer, self.learning_rate, self.eps,
                                         sparse, state, *cores)
        return out.view(shape + (D,))
