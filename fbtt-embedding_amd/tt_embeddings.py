"""`tt_embeddings` -- drop-in for the reference's native extension module.

The reference builds a pybind11/CUDA extension called `tt_embeddings` exporting
eleven functions (reference tt_embeddings.cpp:131-161).  This module exports the
same eleven names with the same positional arguments, tensor conventions and
error behaviour (RuntimeError where the reference's TORCH_CHECK fires), and
forwards every call to the hand-written HIP library `libttx.so` (gfx950) through
its C ABI (include/ttx.h) with ctypes.  PyTorch is used only for device memory
and the current HIP stream.

There is NO CPU or PyTorch fallback: if `libttx.so` is missing, or a tensor is
not on a GPU, the call raises.

Extras beyond the reference's eleven names (used by tt_embeddings_ops.py and
bench.py): `make_plan` (share the lookup plan between forward and backward; `dedup=True`: duplicate lookups of
the batch share one contraction),
`profile_*` (live kernel timings), `lib()` (the loaded ctypes library), the pooling modes' `bag_mean_scale`, `tt_rows_p`,
`bag_max_pool`, `bag_max_pool_backward` and `tt_backward_rows`, padded bags' `bags_compact`, the unpooled lookup's `rows_expand` /
`rows_collect` (and, with a live cache, `preprocess_indices_async`, `rows_place` / `rows_pick`), `bags_merge` (the per-table
batches of a mixed-cardinality group -> one table-major batch, one launch), and the row cache over several tables' `table_keys`,
`table_keys_split` and `cache_populate_tables`, `cache_carry` (trained cache rows and their state across a re-populate), the
dense member tables' `dense_bags_forward` / `dense_bags_backward`, and `adam_apply` (one fused Adam / AdamW step over a list of
dense tensors: OptimType.EXACT_ADAM).
"""
import ctypes as C
import os
import struct
from typing import List, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.environ.get("TTX_LIB") or os.path.join(_HERE, "libttx.so")  # TTX_LIB: try another build of the same library

MAX_CORES = 4
OPTIM_SGD, OPTIM_ADAGRAD, OPTIM_DENSE = 0, 1, 2
PROF_FWD, PROF_BWD, PROF_APPLY, PROF_PLAN, PROF_POOL, PROF_CACHE_FWD = range(6)
FUSED_CACHE_UPDATE = True  # preprocess_indices_sync(..., update_cache_freq=) exists


class _Geom(C.Structure):
    _fields_ = [
        ("T", C.c_int32),
        ("num_tables", C.c_int32),
        ("p", C.c_int32 * MAX_CORES),
        ("q", C.c_int32 * MAX_CORES),
        ("r", C.c_int32 * (MAX_CORES + 1)),
        ("p_tables", C.POINTER(C.c_int32)),  # NULL, or [num_tables][T]: tables of different row factors
    ]


_lib = None        # the library calls go to: the product build, or the test build while a knob is away from its default
_product = None    # libttx.so
_hooks = None      # libttx_hooks.so (same sources, -DTTX_TEST_HOOKS): loaded on the first use of a test / ablation knob
_SO_HOOKS = os.environ.get("TTX_LIB_HOOKS") or os.path.join(_HERE, "libttx_hooks.so")


def lib():
    """libttx.so, loaded once.  Raises RuntimeError if it has not been built.  (While a test / ablation knob is away from
    its default -- debug_skip(), set_chunk(), debug_lds_budget(), ... below -- calls go to libttx_hooks.so instead: the
    product library has no knobs.)"""
    global _lib, _product
    if _lib is not None:
        return _lib
    _product = _load(_SO)
    _lib = _product
    if os.environ.get("TTX_LDS_BUDGET"):  # experiments: LDS budget of the generic kernels' tile search (bytes)
        debug_lds_budget(int(os.environ["TTX_LDS_BUDGET"]))
    if os.environ.get("TTX_DEBUG_SKIP"):  # ablation runs (scripts/upper_bounds.py): results INVALID while set
        debug_skip(int(os.environ["TTX_DEBUG_SKIP"]))
    return _lib


def hooks_lib():
    """libttx_hooks.so (the test build: include/ttx_test_hooks.h), loaded once; calls are routed to it from now on and back
    to the product library as soon as every knob is at its default again (`_knobs_changed`)."""
    global _lib, _hooks
    lib()
    if _hooks is None:
        _hooks = _load(_SO_HOOKS)
        if not _hooks.ttx_has_test_hooks():
            raise RuntimeError(f"tt_embeddings: {_SO_HOOKS} was built without -DTTX_TEST_HOOKS")
        i32 = C.c_int32
        _hooks.ttx_set_chunk.argtypes = [i32]
        _hooks.ttx_debug_lds_budget.argtypes = [i32]
        _hooks.ttx_debug_skip.argtypes = [i32]
        _hooks.ttx_debug_cache_fwd.argtypes = [i32]
        _hooks.ttx_debug_stamps.argtypes = [C.c_void_p]
        _hooks.ttx_debug_plan_layout.argtypes = [C.POINTER(_Geom), C.c_int64, C.POINTER(C.c_int64)]
        _hooks.ttx_debug_plan_route.argtypes = []
    _lib = _hooks
    return _hooks


def _knobs_changed() -> None:
    global _lib
    if _hooks is not None and _lib is _hooks and not _hooks.ttx_debug_state():
        _lib = _product


def _load(path):
    if not os.path.exists(path):
        raise RuntimeError(
            f"tt_embeddings: the HIP library {path} is missing -- build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc --offload-arch=gfx950). "
            "There is no CPU / PyTorch fallback."
        )
    L = C.CDLL(path)
    L.ttx_last_error.restype = C.c_char_p
    for name in (
        "ttx_plan_bytes",
        "ttx_tt_forward_workspace_bytes",
        "ttx_tt_backward_workspace_bytes",
        "ttx_preprocess_workspace_bytes",
        "ttx_cache_populate_workspace_bytes",
    ):
        getattr(L, name).restype = C.c_size_t
    vp, i32, i64, f32, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t
    G = C.POINTER(_Geom)
    L.ttx_plan_bytes.argtypes = [G, i64]
    L.ttx_plan_build.argtypes = [G, i64, vp, vp, vp, vp, sz, vp]
    L.ttx_tt_forward_workspace_bytes.argtypes = [G, i32, i32, i64]
    L.ttx_tt_forward.argtypes = [G, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_tt_forward_o.argtypes = [G, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_tt_forward_arrive_ints.argtypes = [G, i64]
    L.ttx_tt_forward_arrive_ints.restype = i64
    L.ttx_tt_rows.argtypes = [G, i32, i64, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_tt_backward_workspace_bytes.argtypes = [G, i32, i32, i64]
    L.ttx_tt_backward.argtypes = [G, i32, i32, i32, f32, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_split0_expand.argtypes = [i64, i64, i32, i64, vp, vp, vp, vp, vp]
    L.ttx_tt_backward_w.argtypes = [G, i32, i32, i32, f32, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_update_cache_state.argtypes = [i64, vp, i64, vp, vp, vp]
    L.ttx_preprocess_workspace_bytes.argtypes = [i64]
    L.ttx_preprocess_indices_sync.argtypes = [i64, vp, i64, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp,
                                              C.POINTER(i32), C.POINTER(i32), vp, sz, vp]
    L.ttx_preprocess_indices_sync_fused.argtypes = [i64, vp, i64, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp,
                                                    C.POINTER(i32), C.POINTER(i32), vp, vp, vp, sz, vp]
    L.ttx_lookup_prologue.argtypes = [C.POINTER(_Geom), i64, vp, i64, vp, i64, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_cache_populate_workspace_bytes.argtypes = [G, i64, i64, i32]
    L.ttx_cache_populate.argtypes = [G, vp, i64, vp, vp, vp, i64, i32, vp, vp, sz, vp]
    L.ttx_cache_forward.argtypes = [i32, i64, vp, vp, i32, vp, vp, vp]
    L.ttx_cache_backward_sgd.argtypes = [i64, i32, vp, vp, vp, f32, vp, vp]
    L.ttx_cache_backward_dense.argtypes = [i64, i32, vp, vp, vp, i64, vp, vp]
    L.ttx_cache_backward_rowwise_adagrad_approx.argtypes = [i64, i32, vp, vp, vp, f32, f32, vp, vp, vp]
    L.ttx_profile_enable.argtypes = [C.c_int]
    L.ttx_profile_read.argtypes = [C.c_int, C.POINTER(i64), C.POINTER(C.c_double)]
    L.ttx_debug_state.argtypes = []
    L.ttx_debug_state.restype = C.c_int
    L.ttx_has_test_hooks.argtypes = []
    L.ttx_debug_tiles.argtypes = [G, C.POINTER(i32)]
    L.ttx_cache_populate_f.argtypes = [G, vp, i64, vp, vp, vp, i64, i32, vp, i32, vp, sz, vp]
    L.ttx_cache_backward_sorted_workspace_bytes.restype = C.c_size_t
    L.ttx_cache_backward_sorted_workspace_bytes.argtypes = [i64, i64, i32]
    L.ttx_cache_backward_sorted.argtypes = [i32, i64, vp, i64, i32, vp, vp, vp, f32, f32, i64, vp, vp, vp, sz, vp]
    for name in ("ttx_dedup_bytes", "ttx_tt_forward_dd_workspace_bytes", "ttx_tt_backward_dd_workspace_bytes"):
        getattr(L, name).restype = C.c_size_t
    L.ttx_dedup_bytes.argtypes = [G, i64]
    L.ttx_dedup_build.argtypes = [G, i64, vp, vp, vp, sz, vp, sz, vp]
    L.ttx_tt_forward_dd_workspace_bytes.argtypes = [G, i32, i64]
    L.ttx_tt_forward_dd.argtypes = [G, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_tt_backward_dd_workspace_bytes.argtypes = [G, i32, i64]
    L.ttx_tt_backward_dd.argtypes = [G, i32, i32, i32, f32, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # pooling modes (mean / max)
    L.ttx_bag_mean_scale.argtypes = [i64, i32, vp, vp, vp, vp]
    L.ttx_tt_rows_p.argtypes = [G, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_bag_max_pool.argtypes = [i64, i32, i64, vp, vp, vp, vp, vp]
    L.ttx_bag_max_pool_backward.argtypes = [i64, i32, i64, vp, vp, vp, vp, vp]
    L.ttx_tt_backward_rows_workspace_bytes.restype = C.c_size_t
    L.ttx_tt_backward_rows_workspace_bytes.argtypes = [G, i32, i64]
    L.ttx_tt_backward_rows.argtypes = [G, i32, i32, f32, f32, i64, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    # padded bags (padding_idx)
    L.ttx_bags_compact_workspace_bytes.restype = C.c_size_t
    L.ttx_bags_compact_workspace_bytes.argtypes = [i64, i64]
    L.ttx_bags_compact.argtypes = [i64, i64, vp, vp, i64, i64, vp, vp, vp, vp, sz, vp]
    # unpooled rows at padded positions (TTEmbedding's padding_idx) and the plan of a device-side count
    L.ttx_rows_expand.argtypes = [i64, i32, vp, vp, vp, vp]
    L.ttx_rows_collect.argtypes = [i64, i32, vp, vp, vp, vp]
    L.ttx_plan_build_n.argtypes = [G, i64, vp, vp, vp, vp, vp, sz, vp]
    # unpooled rows with a live cache (TTEmbedding(use_cache=True)): the live preprocess with its split point on the device, the
    # rows between partition order and positions, the cache rows' atomic updates from a device-side split point
    L.ttx_preprocess_indices_async.argtypes = [i64, vp, i64, vp, i32, i32, i64, vp, vp, vp, vp, vp, vp, vp,
                                               C.POINTER(i32), C.POINTER(i32), vp, vp, vp, vp, sz, vp]
    L.ttx_rows_place.argtypes = [i64, i64, i64, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.ttx_rows_pick.argtypes = [i64, i64, i64, vp, i32, vp, vp, vp, vp]
    L.ttx_cache_backward_sgd_n.argtypes = [i64, vp, i32, vp, vp, vp, f32, vp, vp]
    L.ttx_cache_backward_dense_n.argtypes = [i64, vp, i32, vp, vp, vp, i64, vp, vp]
    L.ttx_cache_backward_rowwise_adagrad_approx_n.argtypes = [i64, vp, i32, vp, vp, vp, f32, f32, vp, vp, vp]
    # row cache over several tables: (table, index) <-> key, the populate of any table's rows, the gather behind a device-side split
    L.ttx_table_keys.argtypes = [i64, vp, i32, i64, vp, i64, vp, i64, vp, vp, vp]
    L.ttx_table_keys_split.argtypes = [i64, vp, i32, i64, i64, vp, vp, vp, vp, vp, vp]
    L.ttx_cache_populate_t_workspace_bytes.restype = C.c_size_t
    L.ttx_cache_populate_t_workspace_bytes.argtypes = [G, i64, i64, i32]
    L.ttx_cache_populate_t.argtypes = [G, vp, i64, vp, vp, vp, i64, i32, vp, i64, i32, vp, sz, vp]
    L.ttx_cache_forward_n.argtypes = [i32, i64, vp, vp, vp, i32, vp, vp, vp]
    # ... over tables of different row factors: a host array of num_tables + 1 key bases in the place of the one stride
    L.ttx_table_keys_v.argtypes = [i64, vp, i32, i64, vp, vp, vp, i64, vp, vp, vp]
    L.ttx_table_keys_split_v.argtypes = [i64, vp, i32, i64, vp, vp, vp, vp, vp, vp, vp]
    L.ttx_cache_populate_v_workspace_bytes.restype = C.c_size_t
    L.ttx_cache_populate_v_workspace_bytes.argtypes = [G, i64, i64, i32]
    L.ttx_cache_populate_v.argtypes = [G, vp, i64, vp, vp, vp, i64, i32, vp, i32, vp, sz, vp]
    # cache refresh: trained rows and their optimizer state across a re-populate
    L.ttx_cache_carry.argtypes = [i64, vp, vp, vp, i64, i32, vp, vp, i32, vp, vp, vp]
    # merged bags (per-table batches -> one table-major batch)
    L.ttx_bags_merge.argtypes = [i32, i64, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp]
    # dense member tables (bags over uncompressed rows)
    L.ttx_dense_bags_forward.argtypes = [i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.ttx_dense_bags_backward_workspace_bytes.restype = C.c_size_t
    L.ttx_dense_bags_backward_workspace_bytes.argtypes = [i64, i64, i32]
    L.ttx_dense_bags_backward.argtypes = [i32, i32, i64, i32, i64, vp, vp, vp, vp, vp, i32, vp, vp, vp, f32, f32, i32, vp, vp, vp,
                                          vp, vp, sz, vp]
    L.ttx_dense_bags_info.argtypes = [i32, i64, C.POINTER(i32)]
    # fused Adam over a list of dense tensors
    L.ttx_adam_apply_workspace_bytes.restype = C.c_size_t
    L.ttx_adam_apply_workspace_bytes.argtypes = [i32]
    L.ttx_adam_apply.argtypes = [i32, vp, vp, vp, vp, vp, vp, f32, f32, f32, f32, f32, i32, vp, sz, vp]
    # bf16 inference forward
    L.ttx_tt_rows_bf16_supported.argtypes = [G]
    L.ttx_tt_pack_bf16_elems.restype = i64
    L.ttx_tt_pack_bf16_elems.argtypes = [G, i32]
    L.ttx_tt_pack_bf16.argtypes = [G, i32, vp, vp, vp]
    L.ttx_tt_rows_bf16_workspace_bytes.restype = C.c_size_t
    L.ttx_tt_rows_bf16_workspace_bytes.argtypes = [G, i32, i64]
    L.ttx_tt_rows_bf16.argtypes = [G, i32, i64, vp, vp, vp, vp, vp, vp, sz, vp]
    L.ttx_bag_sum_pool.argtypes = [i64, i32, vp, vp, vp, vp]
    return L


def _check(rc: int) -> None:
    if rc != 0:
        raise RuntimeError("tt_embeddings (libttx): " + lib().ttx_last_error().decode())


_geom_cache = {}


def _geom(num_tables: int, p: Sequence, q: Sequence[int], ranks: Sequence[int]) -> _Geom:
    """`p` = tt_p_shapes, or (beyond the reference: include/ttx.h ttx_geom::p_tables) one list per table for
    tables of different row factors -- the cores are then [1, sum of the tables' p_t, slice]."""
    if len(p) > 0 and isinstance(p[0], (list, tuple)):
        return _geom_mixed(p, q, ranks)
    key = (int(num_tables), tuple(int(x) for x in p), tuple(int(x) for x in q), tuple(int(x) for x in ranks))
    g = _geom_cache.get(key)
    if g is None:
        T = len(key[1])
        if not (2 <= T <= MAX_CORES) or len(key[2]) != T or len(key[3]) != T + 1:
            raise RuntimeError(
                f"tt_embeddings: need 2..4 cores with len(q) == len(p) and len(ranks) == len(p)+1, got "
                f"p={list(key[1])} q={list(key[2])} ranks={list(key[3])}")
        g = _Geom()
        g.T, g.num_tables = T, key[0]
        for t in range(T):
            g.p[t], g.q[t] = key[1][t], key[2][t]
        for t in range(T + 1):
            g.r[t] = key[3][t]
        _geom_cache[key] = g
    return g


def _geom_mixed(p, q, ranks) -> _Geom:
    key = ("mixed", tuple(tuple(int(x) for x in row) for row in p), tuple(int(x) for x in q), tuple(int(x) for x in ranks))
    g = _geom_cache.get(key)
    if g is None:
        T = len(key[2])
        if not (2 <= T <= MAX_CORES) or len(key[3]) != T + 1 or any(len(row) != T for row in key[1]):
            raise RuntimeError(f"tt_embeddings: per-table tt_p_shapes need {T} factors each and len(ranks) == {T + 1}")
        g = _Geom()
        g.T, g.num_tables = T, len(key[1])
        flat = [v for row in key[1] for v in row]
        g._ptab = (C.c_int32 * len(flat))(*flat)  # kept alive by the cached struct
        g.p_tables = C.cast(g._ptab, C.POINTER(C.c_int32))
        g._psum = [sum(row[t] for row in key[1]) for t in range(T)]
        for t in range(T):
            g.p[t], g.q[t] = max(row[t] for row in key[1]), key[2][t]
        for t in range(T + 1):
            g.r[t] = key[3][t]
        _geom_cache[key] = g
    return g


def _dev(t: torch.Tensor) -> torch.device:
    if not t.is_cuda:
        raise RuntimeError("tt_embeddings: tensors must live on a GPU (no CPU path in this build)")
    return t.device


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(dev: torch.device) -> int:
    """the current HIP stream of `dev` as an integer handle (the raw getter skips building a
    torch.cuda.Stream object: ~8 us per call on the lookup path)"""
    if _raw_stream is not None:
        return _raw_stream(dev.index if dev.index is not None else torch.cuda.current_device())
    return torch.cuda.current_stream(dev).cuda_stream


class _guard:
    """OptionalCUDAGuard of the reference entry points (e.g. cu:436-437)."""

    __slots__ = ("dev", "prev")

    def __init__(self, dev):
        self.dev = dev.index if dev.index is not None else torch.cuda.current_device()
        self.prev = None

    def __enter__(self):
        cur = torch.cuda.current_device()
        if cur != self.dev:
            self.prev = cur
            torch.cuda.set_device(self.dev)

    def __exit__(self, *a):
        if self.prev is not None:
            torch.cuda.set_device(self.prev)


_ws_cache = {}


def _workspace(dev: torch.device, stream: int, nbytes: int) -> torch.Tensor:
    """Grow-only scratch per (device, stream): stream order makes reuse safe."""
    key = (dev.index, stream)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(int(nbytes * 1.25), 1 << 20), dtype=torch.uint8, device=dev)
        _ws_cache[key] = ws
    return ws


_arrive_cache = {}


def _arrive_zeros(dev: torch.device, stream: int, n: int) -> torch.Tensor:
    """the arrival counters of fused pooling: zero before and after every call, so one array per (device, stream)"""
    key = (dev.index, stream)
    t = _arrive_cache.get(key)
    if t is None or t.numel() < n:
        t = torch.zeros(max(n, 1 << 16), dtype=torch.int32, device=dev)
        _arrive_cache[key] = t
    return t


def _ptr_array(tensors: Sequence[torch.Tensor]):
    arr = (C.c_void_p * len(tensors))()
    for i, t in enumerate(tensors):
        arr[i] = t.data_ptr()
    return arr


def _i64(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.int64:
        raise RuntimeError(f"tt_embeddings: {name} must be int64, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _f32(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32:
        raise RuntimeError(f"tt_embeddings: {name} must be float32, got {t.dtype}")
    return t if t.is_contiguous() else t.contiguous()


def _cores(tt_cores: Sequence[torch.Tensor], g: _Geom, name="tt_cores"):
    if len(tt_cores) != g.T:
        raise RuntimeError(f"tt_embeddings: expected {g.T} {name}, got {len(tt_cores)}")
    out = []
    for t, c in enumerate(tt_cores):
        c = c.detach() if c.requires_grad else c
        want = (g.num_tables, g.p[t], g.r[t] * g.q[t] * g.r[t + 1])
        if bool(g.p_tables):  # tables of different row factors: one array of all their slices
            want = (1, g._psum[t], want[2])
        if tuple(c.shape) != want or c.dtype != torch.float32 or not c.is_contiguous() or not c.is_cuda:
            raise RuntimeError(f"tt_embeddings: {name}[{t}] must be a contiguous float32 GPU tensor of shape {want}, "
                               f"got {tuple(c.shape)} {c.dtype} on {c.device}")
        out.append(c)
    return out


class Plan:
    """Device-resident lookup plan shared by forward and backward of one batch."""

    __slots__ = ("buf", "nnz", "key")

    def __init__(self, buf, nnz, key):
        self.buf, self.nnz, self.key = buf, nnz, key


class DedupPlan(Plan):
    """A plan of the batch's DISTINCT (table, index) pairs plus the map of the lookups onto them (include/ttx.h,
    "duplicate lookups"): tt_forward / the backward entry points given such a plan contract every distinct pair
    once.  Built by make_plan(..., dedup=True) when the batch qualifies."""

    __slots__ = ("dd",)

    def __init__(self, buf, dd, nnz, key):
        super().__init__(buf, nnz, key)
        self.dd = dd


def make_plan(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, nnz, indices, tableidx, rowidx=None,
              dedup: bool = False, n_dev: Optional[torch.Tensor] = None) -> Optional[Plan]:
    """`n_dev` (trailing keyword): one int32 on the device, the number of LEADING entries of indices / tableidx / rowidx to plan
    (<= nnz, which then only sizes the plan: ttx_plan_build_n) -- no host read-back of the count."""
    if nnz == 0:
        return None
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(indices)
    indices, tableidx = _i64(indices, "indices"), _i64(tableidx, "tableidx")
    L = lib()
    if n_dev is not None:
        if dedup:
            raise RuntimeError("tt_embeddings: make_plan(dedup=True) does not take a device-side count")
        if n_dev.dtype != torch.int32 or n_dev.numel() != 1 or n_dev.device != dev:
            raise RuntimeError(f"tt_embeddings: n_dev must be one int32 on {dev}, got {n_dev.dtype} x {n_dev.numel()} on {n_dev.device}")
        if indices.numel() < nnz or tableidx.numel() < nnz or (rowidx is not None and rowidx.numel() < nnz):
            raise RuntimeError("tt_embeddings: nnz exceeds the index tensors")
        nb = L.ttx_plan_bytes(C.byref(g), nnz)
        buf = torch.empty(nb, dtype=torch.uint8, device=dev)
        with _guard(dev):
            _check(L.ttx_plan_build_n(C.byref(g), nnz, n_dev.data_ptr(), indices.data_ptr(), tableidx.data_ptr(),
                                      None if rowidx is None else _i64(rowidx, "rowidx").data_ptr(), buf.data_ptr(), nb,
                                      _stream(dev)))
        return Plan(buf, nnz, (num_tables, tuple(tt_p_shapes), tuple(tt_q_shapes), tuple(tt_ranks)))
    if dedup:
        db = L.ttx_dedup_bytes(C.byref(g), nnz)
        if db:  # (0: tables of different row factors, or tables * prod(p) beyond 2^61 -- the plain plan gives the same results;
            #  batches of any size and key spaces beyond 2^32 ARE mapped: csrc/ttx_plan.hip dedup_build_large)
            nb = L.ttx_plan_bytes(C.byref(g), nnz)
            buf = torch.empty(nb, dtype=torch.uint8, device=dev)
            dd = torch.empty(db, dtype=torch.uint8, device=dev)
            with _guard(dev):
                _check(L.ttx_dedup_build(C.byref(g), nnz, indices.data_ptr(), tableidx.data_ptr(), dd.data_ptr(), db,
                                         buf.data_ptr(), nb, _stream(dev)))
            return DedupPlan(buf, dd, nnz, (num_tables, tuple(tt_p_shapes), tuple(tt_q_shapes), tuple(tt_ranks)))
    nb = L.ttx_plan_bytes(C.byref(g), nnz)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(L.ttx_plan_build(C.byref(g), nnz, indices.data_ptr(), tableidx.data_ptr(),
                                None if rowidx is None else _i64(rowidx, "rowidx").data_ptr(), buf.data_ptr(), nb, _stream(dev)))
    return Plan(buf, nnz, (num_tables, tuple(tt_p_shapes), tuple(tt_q_shapes), tuple(tt_ranks)))


def split0_expand(indices: torch.Tensor, offsets: torch.Tensor, k: int, p_rest: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Not in the reference: the part lookups of a table whose first factor is split k ways (include/ttx.h, "core-0 row
    split").  offsets: nb + 1 entries.  -> (indices [k nnz], offsets [k nb + 1])."""
    dev = _dev(indices)
    indices, offsets = _i64(indices, "indices"), _i64(offsets, "offsets")
    nnz, nb = indices.numel(), offsets.numel() - 1
    out_i = torch.empty(k * nnz, dtype=torch.int64, device=dev)
    out_o = torch.empty(k * nb + 1, dtype=torch.int64, device=dev)
    with _guard(dev):
        _check(lib().ttx_split0_expand(nnz, nb, k, p_rest, indices.data_ptr(), offsets.data_ptr(), out_i.data_ptr(),
                                       out_o.data_ptr(), _stream(dev)))
    return out_i, out_o


def lookup_prologue(colidx: torch.Tensor, offsets: torch.Tensor, num_tables: int, tt_p_shapes, tt_q_shapes, tt_ranks,
                    hashtbl: Optional[torch.Tensor] = None, cache_freq: Optional[torch.Tensor] = None
                    ) -> Tuple[torch.Tensor, torch.Tensor, Optional[Plan]]:
    """Not in the reference: update_cache_state (when hashtbl / cache_freq are given) +
    preprocess_indices_sync(warmup=True) + make_plan of one batch in ONE native call (one launch
    when the batch qualifies, include/ttx.h).  -> (rowidx, tableidx, plan)."""
    dev = _dev(colidx)
    colidx, offsets = _i64(colidx, "colidx"), _i64(offsets, "offsets")
    nnz = colidx.numel()
    rowidx = torch.empty_like(colidx)
    tableidx = torch.empty_like(colidx)
    if nnz == 0:
        return rowidx, tableidx, None
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    upd = hashtbl is not None and cache_freq is not None and hashtbl.numel() > 0
    if upd and hashtbl.numel() != cache_freq.numel():
        raise RuntimeError("tt_embeddings: hashtbl must match cache_freq")
    L = lib()
    nb = L.ttx_plan_bytes(C.byref(g), nnz)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(L.ttx_lookup_prologue(C.byref(g), nnz, colidx.data_ptr(), offsets.numel() - 1, offsets.data_ptr(),
                                     hashtbl.numel() if upd else 0, hashtbl.data_ptr() if upd else None,
                                     cache_freq.data_ptr() if upd else None, rowidx.data_ptr(), tableidx.data_ptr(),
                                     buf.data_ptr(), nb, _stream(dev)))
    return rowidx, tableidx, Plan(buf, nnz, (num_tables, tuple(tt_p_shapes), tuple(tt_q_shapes), tuple(tt_ranks)))


def _plan_ptr(plan: Optional[Plan], nnz: int):
    if plan is None:
        return None
    if plan.nnz != nnz:
        raise RuntimeError("tt_embeddings: plan was built for a different nnz")
    return plan.buf.data_ptr()


# --------------------------------------------------------------------------- #
# the eleven reference entry points (tt_embeddings.cpp:131-161)
# --------------------------------------------------------------------------- #

def tt_forward(batch_count: int, num_tables: int, B: int, D: int, tt_p_shapes: List[int], tt_q_shapes: List[int],
               tt_ranks: List[int], L: torch.Tensor, nnz: int, indices: torch.Tensor, rowidx: torch.Tensor,
               tableidx: torch.Tensor, tt_cores: List[torch.Tensor], plan: Optional[Plan] = None,
               offsets: Optional[torch.Tensor] = None, per_sample_weights: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tt_embeddings.cpp:13-26.  `batch_count` (the reference's GEMM chunk size)
    is accepted and ignored: the HIP path has no chunk loop.  `L` is validated
    for length only; strides are derived from tt_p_shapes."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(tt_cores[0])
    cores = _cores(tt_cores, g)
    out = torch.empty((num_tables, B, D), dtype=torch.float32, device=dev)
    if nnz > 0 and batch_count <= 0:
        raise RuntimeError("tt_embeddings: batch_count must be > 0")  # cu:987
    if L.numel() != g.T:
        raise RuntimeError("tt_embeddings: L must have one stride per core")
    indices, rowidx, tableidx = _i64(indices, "indices"), _i64(rowidx, "rowidx"), _i64(tableidx, "tableidx")
    if nnz > indices.numel() or nnz > rowidx.numel() or nnz > tableidx.numel():
        raise RuntimeError("tt_embeddings: nnz exceeds the index tensors")
    lb = lib()
    st = _stream(dev)
    if isinstance(plan, DedupPlan) and nnz > 0:
        nb = lb.ttx_tt_forward_dd_workspace_bytes(C.byref(g), D, nnz)
        ws = _workspace(dev, st, nb)
        with _guard(dev):
            psw = None if per_sample_weights is None else _f32(per_sample_weights, "per_sample_weights")
            _check(lb.ttx_tt_forward_dd(C.byref(g), B, D, nnz, rowidx.data_ptr(), tableidx.data_ptr(),
                                        None if psw is None else psw.data_ptr(), plan.dd.data_ptr(),
                                        _plan_ptr(plan, nnz), _ptr_array(cores), out.data_ptr(), ws.data_ptr(), ws.numel(), st))
        return out
    nb = lb.ttx_tt_forward_workspace_bytes(C.byref(g), B, D, nnz)
    ws = _workspace(dev, st, nb)
    if offsets is not None or per_sample_weights is not None:
        # beyond the reference's signature: the bags' offsets (the ones rowidx / tableidx were derived from) let the
        # contraction kernel pool the bags itself (include/ttx.h ttx_tt_forward_o) -- same output bit for bit
        na = lb.ttx_tt_forward_arrive_ints(C.byref(g), nnz) if (offsets is not None and nnz > 0) else 0
        arrive = _arrive_zeros(dev, st, na) if na > 0 else None
        psw = None if per_sample_weights is None else _f32(per_sample_weights, "per_sample_weights")
        with _guard(dev):
            _check(lb.ttx_tt_forward_o(C.byref(g), B, D, nnz, indices.data_ptr(), rowidx.data_ptr(), tableidx.data_ptr(),
                                       None if psw is None else psw.data_ptr(), _ptr_array(cores), out.data_ptr(), None,
                                       _i64(offsets, "offsets").data_ptr() if na > 0 else None,
                                       arrive.data_ptr() if na > 0 else None, _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
        return out
    with _guard(dev):
        _check(lb.ttx_tt_forward(C.byref(g), B, D, nnz, indices.data_ptr(), rowidx.data_ptr(), tableidx.data_ptr(),
                                 _ptr_array(cores), out.data_ptr(), _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
    return out


def _backward(optim, D, lr, eps, p, q, ranks, nnz, indices, rowidx, tableidx, d_output, tt_cores, state, plan,
              per_sample_weights=None):
    g = _geom(tt_cores[0].size(0), p, q, ranks)
    num_tables = g.num_tables  # (tables of different row factors: len(p), the cores are [1, sum p, slice])
    dev = _dev(d_output)
    cores = _cores(tt_cores, g)
    d_output = _f32(d_output, "d_output")
    if d_output.dim() != 3 or d_output.size(0) != num_tables or d_output.size(2) != D:
        raise RuntimeError(f"tt_embeddings: d_output must be [num_tables, B, D], got {tuple(d_output.shape)}")
    B = d_output.size(1)
    indices, rowidx, tableidx = _i64(indices, "indices"), _i64(rowidx, "rowidx"), _i64(tableidx, "tableidx")
    grads = None
    gptr = sptr = None
    if optim == OPTIM_DENSE:
        grads = [torch.empty_like(c) for c in cores]
        gptr = _ptr_array(grads)
    if optim == OPTIM_ADAGRAD:
        sptr = _ptr_array(_cores(state, g, "optimizer_state"))
    lb = lib()
    st = _stream(dev)
    # (beyond the reference's signature: nn.EmbeddingBag's per_sample_weights scale each lookup's share of its bag gradient)
    psw = None if per_sample_weights is None else _f32(per_sample_weights, "per_sample_weights")
    pswp = None if psw is None else psw.data_ptr()
    if isinstance(plan, DedupPlan) and nnz > 0:
        nb = lb.ttx_tt_backward_dd_workspace_bytes(C.byref(g), D, nnz)
        ws = _workspace(dev, st, nb)
        with _guard(dev):
            _check(lb.ttx_tt_backward_dd(C.byref(g), optim, B, D, lr, eps, nnz, rowidx.data_ptr(), tableidx.data_ptr(), pswp,
                                         d_output.data_ptr(), plan.dd.data_ptr(), _plan_ptr(plan, nnz), _ptr_array(cores), sptr,
                                         gptr, ws.data_ptr(), ws.numel(), st))
        return grads
    nb = lb.ttx_tt_backward_workspace_bytes(C.byref(g), B, D, nnz)
    ws = _workspace(dev, st, nb)
    with _guard(dev):
        if psw is not None:
            _check(lb.ttx_tt_backward_w(C.byref(g), optim, B, D, lr, eps, nnz, indices.data_ptr(), rowidx.data_ptr(),
                                        tableidx.data_ptr(), pswp, d_output.data_ptr(), _ptr_array(cores), sptr, gptr,
                                        _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
        else:
            _check(lb.ttx_tt_backward(C.byref(g), optim, B, D, lr, eps, nnz, indices.data_ptr(), rowidx.data_ptr(),
                                      tableidx.data_ptr(), d_output.data_ptr(), _ptr_array(cores), sptr, gptr,
                                      _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
    return grads


def tt_dense_backward(batch_count, D, tt_p_shapes, tt_q_shapes, tt_ranks, L, nnz, indices, rowidx, tableidx, d_output,
                      tt_cores, plan: Optional[Plan] = None, per_sample_weights: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
    """tt_embeddings.cpp:28-40: returns the list of dense core gradients."""
    return _backward(OPTIM_DENSE, D, 0.0, 0.0, tt_p_shapes, tt_q_shapes, tt_ranks, nnz, indices, rowidx, tableidx,
                     d_output, tt_cores, None, plan, per_sample_weights)


def tt_sgd_backward(batch_count, D, learning_rate, tt_p_shapes, tt_q_shapes, tt_ranks, L, nnz, indices, rowidx,
                    tableidx, d_output, tt_cores, plan: Optional[Plan] = None,
                    per_sample_weights: Optional[torch.Tensor] = None) -> None:
    """tt_embeddings.cpp:42-55: fused gradient + SGD, cores updated in place."""
    _backward(OPTIM_SGD, D, learning_rate, 0.0, tt_p_shapes, tt_q_shapes, tt_ranks, nnz, indices, rowidx, tableidx,
              d_output, tt_cores, None, plan, per_sample_weights)


def tt_adagrad_backward(batch_count, D, learning_rate, eps, tt_p_shapes, tt_q_shapes, tt_ranks, L, nnz, indices,
                        rowidx, tableidx, d_output, optimizer_state, tt_cores, plan: Optional[Plan] = None,
                        per_sample_weights: Optional[torch.Tensor] = None) -> None:
    """tt_embeddings.cpp:57-72: fused gradient + Adagrad, cores and state in place."""
    _backward(OPTIM_ADAGRAD, D, learning_rate, eps, tt_p_shapes, tt_q_shapes, tt_ranks, nnz, indices, rowidx,
              tableidx, d_output, tt_cores, list(optimizer_state), plan, per_sample_weights)


def update_cache_state(indices: torch.Tensor, hashtbl: torch.Tensor, cache_freq: torch.Tensor) -> None:
    """tt_embeddings.cpp:74."""
    nnz = indices.numel()
    if nnz == 0:
        return
    dev = _dev(indices)
    if hashtbl.numel() <= 0 or hashtbl.numel() != cache_freq.numel():  # cu:1099-1100
        raise RuntimeError("tt_embeddings: hashtbl must be non-empty and match cache_freq")
    indices = _i64(indices, "indices")
    _i64(hashtbl, "hashtbl"), _i64(cache_freq, "cache_freq")
    with _guard(dev):
        _check(lib().ttx_update_cache_state(nnz, indices.data_ptr(), hashtbl.numel(), hashtbl.data_ptr(),
                                            cache_freq.data_ptr(), _stream(dev)))


def cache_populate(num_embeddings: int, tt_p_shapes, tt_q_shapes, tt_ranks, tt_cores, L, hashtbl, cache_freq,
                   cache_state, cache_weight, reference_exact: bool = False) -> None:
    """tt_embeddings.cpp:76-86.  `reference_exact` (trailing keyword, not in the reference): leave the cache_state of evicted
    slots untouched, as the reference's mark_popular_colidx_kernel does (include/ttx.h TTX_POPULATE_REFERENCE_EXACT)."""
    g = _geom(tt_cores[0].size(0), tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(cache_weight)
    cores = _cores(list(tt_cores), g)
    H = hashtbl.numel()
    if H <= 0 or H != cache_freq.numel() or H < cache_weight.size(0):  # cu:1271-1274
        raise RuntimeError("tt_embeddings: need 0 < hashtbl.numel() == cache_freq.numel() >= cache_size")
    if cache_state.dtype != torch.int32 or cache_state.numel() != H:
        raise RuntimeError("tt_embeddings: cache_state must be int32[hashtbl_size]")
    cw = cache_weight.detach()
    if cw.dtype != torch.float32 or not cw.is_contiguous():
        raise RuntimeError("tt_embeddings: cache_weight must be contiguous float32")
    cs, D = cw.size(0), cw.size(1)
    lb = lib()
    st = _stream(dev)
    nb = lb.ttx_cache_populate_workspace_bytes(C.byref(g), H, cs, D)
    ws = _workspace(dev, st, nb)
    with _guard(dev):
        _check(lb.ttx_cache_populate_f(C.byref(g), _ptr_array(cores), H, hashtbl.data_ptr(), cache_freq.data_ptr(),
                                       cache_state.data_ptr(), cs, D, cw.data_ptr(), 1 if reference_exact else 0,
                                       ws.data_ptr(), ws.numel(), st))


def _key_bases(key_stride, num_tables: int):
    """`key_stride` of table_keys / table_keys_split: an int is the one stride of tables of one row shape (-> None); a sequence
    is the num_tables + 1 key bases of tables of different row factors (-> the host int64 array the `_v` calls read)."""
    if hasattr(key_stride, "__index__"):  # (an int, numpy's integers)
        return None
    bases = [int(v) for v in key_stride]
    if len(bases) != num_tables + 1:
        raise RuntimeError(f"tt_embeddings: {num_tables} tables need {num_tables + 1} key bases, got {len(bases)}")
    return (C.c_int64 * len(bases))(*bases)


def key_bases_of(tt_p_shapes) -> List[int]:
    """the key bases of tables of different row factors (include/ttx.h, "row cache over tables of different row factors"):
    the running sum of the tables' prod(p), num_tables + 1 entries, the last one the size of the key space"""
    bases = [0]
    for p in tt_p_shapes:
        rows = 1
        for v in p:
            rows *= int(v)
        bases.append(bases[-1] + rows)
    return bases


def table_keys(indices: torch.Tensor, offsets: torch.Tensor, num_tables: int, key_stride,
               hashtbl: Optional[torch.Tensor] = None, cache_freq: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Not in the reference: the keys of a table-major batch in the row cache over several tables (include/ttx.h, "row cache
    over several tables") -- keys[n] = indices[n] + table(n) * key_stride, the table read off the batch's bag `offsets`
    (num_tables * B + 1 entries, closing entry included).  With `hashtbl` / `cache_freq` the same launch counts the keys, as
    update_cache_state(keys, hashtbl, cache_freq) would.  `key_stride` may be a sequence of num_tables + 1 key bases instead
    (tables of different row factors, `key_bases_of`): keys[n] = indices[n] + key_stride[table(n)] (ttx_table_keys_v).
    -> keys [nnz] int64."""
    dev = _dev(indices)
    indices, offsets = _i64(indices, "indices"), _i64(offsets, "offsets")
    nnz, nb = indices.numel(), offsets.numel() - 1
    if num_tables <= 0 or nb <= 0 or nb % num_tables != 0 or offsets.device != dev:
        raise RuntimeError(f"tt_embeddings: offsets must hold num_tables * B + 1 entries on {dev}, got {offsets.numel()} for "
                           f"{num_tables} tables on {offsets.device}")
    count = hashtbl is not None or cache_freq is not None
    if count:
        if hashtbl is None or cache_freq is None or hashtbl.numel() <= 0 or hashtbl.numel() != cache_freq.numel():
            raise RuntimeError("tt_embeddings: hashtbl must be non-empty and match cache_freq")
        _i64(hashtbl, "hashtbl"), _i64(cache_freq, "cache_freq")
        if hashtbl.device != dev or cache_freq.device != dev:
            raise RuntimeError(f"tt_embeddings: hashtbl and cache_freq must be on {dev}")
    bases = _key_bases(key_stride, num_tables)
    keys = torch.empty_like(indices)
    if nnz == 0:
        return keys
    with _guard(dev):
        call = lib().ttx_table_keys if bases is None else lib().ttx_table_keys_v
        _check(call(nnz, indices.data_ptr(), num_tables, nb // num_tables, offsets.data_ptr(),
                    int(key_stride) if bases is None else bases, keys.data_ptr(), hashtbl.numel() if count else 0,
                    hashtbl.data_ptr() if count else None, cache_freq.data_ptr() if count else None, _stream(dev)))
    return keys


def table_keys_split(keys: torch.Tensor, bagrow: Optional[torch.Tensor], num_tables: int, B: int, key_stride,
                     n_dev: Optional[torch.Tensor] = None
                     ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Not in the reference: the inverse of table_keys on the first *n_dev entries (one int32 on the device; None: all).  With
    `bagrow` (flat bag rows table * B + b: the prow of preprocess_indices_async over keys) -> (indices, tableidx, rowidx) of
    those entries, what make_plan(n_dev=) takes for the misses; with bagrow None the table is keys // key_stride and rowidx is
    None.  Entries at and beyond the count are not written (uninitialised).  `key_stride` may be a sequence of num_tables + 1
    key bases instead (ttx_table_keys_split_v): with bagrow None the table is then the last one whose base is <= the key."""
    dev = _dev(keys)
    keys = _i64(keys, "keys")
    n = keys.numel()
    bases = _key_bases(key_stride, num_tables)
    out_i, out_t = torch.empty_like(keys), torch.empty_like(keys)
    out_r = None
    if bagrow is not None:
        bagrow = _i64(bagrow, "bagrow")
        if bagrow.numel() < n or bagrow.device != dev:
            raise RuntimeError(f"tt_embeddings: bagrow must hold one bag row per key on {dev}")
        out_r = torch.empty_like(keys)
    if n == 0:
        return out_i, out_t, out_r
    with _guard(dev):
        call = lib().ttx_table_keys_split if bases is None else lib().ttx_table_keys_split_v
        _check(call(n, None if n_dev is None else _skip_ptr(n_dev, dev), num_tables, B, int(key_stride) if bases is None else bases,
                    keys.data_ptr(), None if bagrow is None else bagrow.data_ptr(), out_i.data_ptr(), out_t.data_ptr(),
                    None if out_r is None else out_r.data_ptr(), _stream(dev)))
    return out_i, out_t, out_r


def cache_populate_tables(num_tables: int, tt_p_shapes, tt_q_shapes, tt_ranks, tt_cores, hashtbl, cache_freq, cache_state,
                          cache_weight, key_stride: int, reference_exact: bool = False) -> None:
    """Not in the reference: cache_populate for the row cache over the `num_tables` tables of one table-batched bag, whose
    hash table holds keys table * key_stride + index (ttx_cache_populate_t): the cache_size most frequent keys get the cache
    rows, each decompressed from its own table's cores."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(cache_weight)
    cores = _cores(list(tt_cores), g)
    H = hashtbl.numel()
    if H <= 0 or H != cache_freq.numel() or H < cache_weight.size(0):
        raise RuntimeError("tt_embeddings: need 0 < hashtbl.numel() == cache_freq.numel() >= cache_size")
    _i64(hashtbl, "hashtbl"), _i64(cache_freq, "cache_freq")
    if cache_state.dtype != torch.int32 or cache_state.numel() != H:
        raise RuntimeError("tt_embeddings: cache_state must be int32[hashtbl_size]")
    cw = cache_weight.detach()
    if cw.dtype != torch.float32 or not cw.is_contiguous():
        raise RuntimeError("tt_embeddings: cache_weight must be contiguous float32")
    cs, D = cw.size(0), cw.size(1)
    lb = lib()
    st = _stream(dev)
    nb = lb.ttx_cache_populate_t_workspace_bytes(C.byref(g), H, cs, D)
    ws = _workspace(dev, st, nb)
    with _guard(dev):
        _check(lb.ttx_cache_populate_t(C.byref(g), _ptr_array(cores), H, hashtbl.data_ptr(), cache_freq.data_ptr(),
                                       cache_state.data_ptr(), cs, D, cw.data_ptr(), int(key_stride),
                                       1 if reference_exact else 0, ws.data_ptr(), ws.numel(), st))


def cache_populate_var_tables(tt_p_shapes, tt_q_shapes, tt_ranks, tt_cores, hashtbl, cache_freq, cache_state, cache_weight,
                              reference_exact: bool = False) -> None:
    """Not in the reference: cache_populate for the row cache over tables of DIFFERENT row factors (`tt_p_shapes`: one list per
    table; cores [1, sum_k p_k_t, slice]), whose hash table holds keys key_bases_of(tt_p_shapes)[table] + index
    (ttx_cache_populate_v): the cache_size most frequent keys get the cache rows, each decompressed from its own table's cores."""
    if len(tt_p_shapes) == 0 or not isinstance(tt_p_shapes[0], (list, tuple)):
        raise RuntimeError("tt_embeddings: cache_populate_var_tables takes one list of row factors per table")
    g = _geom_mixed(tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(cache_weight)
    cores = _cores(list(tt_cores), g)
    H = hashtbl.numel()
    if H <= 0 or H != cache_freq.numel() or H < cache_weight.size(0):
        raise RuntimeError("tt_embeddings: need 0 < hashtbl.numel() == cache_freq.numel() >= cache_size")
    _i64(hashtbl, "hashtbl"), _i64(cache_freq, "cache_freq")
    if cache_state.dtype != torch.int32 or cache_state.numel() != H:
        raise RuntimeError("tt_embeddings: cache_state must be int32[hashtbl_size]")
    cw = cache_weight.detach()
    if cw.dtype != torch.float32 or not cw.is_contiguous():
        raise RuntimeError("tt_embeddings: cache_weight must be contiguous float32")
    cs, D = cw.size(0), cw.size(1)
    lb = lib()
    st = _stream(dev)
    with _guard(dev):
        nb = lb.ttx_cache_populate_v_workspace_bytes(C.byref(g), H, cs, D)
        ws = _workspace(dev, st, nb)
        _check(lb.ttx_cache_populate_v(C.byref(g), _ptr_array(cores), H, hashtbl.data_ptr(), cache_freq.data_ptr(),
                                       cache_state.data_ptr(), cs, D, cw.data_ptr(), 1 if reference_exact else 0,
                                       ws.data_ptr(), ws.numel(), st))


def cache_carry(hashtbl: torch.Tensor, old_state: torch.Tensor, cache_state: torch.Tensor, old_weight: torch.Tensor,
                cache_weight: torch.Tensor, old_opt_state: Optional[torch.Tensor] = None,
                opt_state: Optional[torch.Tensor] = None) -> None:
    """Not in the reference: after a populate (any of the three above), move what the cache had learnt to where it now belongs
    (ttx_cache_carry).  `old_state` / `old_weight` / `old_opt_state` are copies of cache_state / cache_weight / the cache rows'
    optimizer state taken BEFORE the populate.  A key cached before and after gets its old row and state in its new row; a key
    new to the cache keeps the decompressed row and zero state; rows no key owns are not written.  The state is [cache_size]
    (row-wise) or [cache_size, D] (element-wise), both or neither given."""
    dev = _dev(cache_weight)
    _i64(hashtbl, "hashtbl")
    H = hashtbl.numel()
    cw, ow = cache_weight.detach(), old_weight.detach()
    for name, t in (("cache_weight", cw), ("old_weight", ow)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
            raise RuntimeError(f"tt_embeddings: {name} must be contiguous float32 [cache_size, D]")
    if ow.shape != cw.shape:
        raise RuntimeError("tt_embeddings: old_weight must have cache_weight's shape")
    cs, D = cw.size(0), cw.size(1)
    if H <= 0 or H < cs or not hashtbl.is_contiguous():
        raise RuntimeError("tt_embeddings: need a contiguous hashtbl with 0 < hashtbl.numel() >= cache_size")
    for name, t in (("cache_state", cache_state), ("old_state", old_state)):
        if t.dtype != torch.int32 or t.numel() != H or not t.is_contiguous():
            raise RuntimeError(f"tt_embeddings: {name} must be contiguous int32[hashtbl_size]")
    width, sp, osp = 0, None, None
    if (opt_state is None) != (old_opt_state is None):
        raise RuntimeError("tt_embeddings: opt_state and old_opt_state go together")
    if opt_state is not None:
        for name, t in (("opt_state", opt_state), ("old_opt_state", old_opt_state)):
            if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) not in ((cs,), (cs, D)):
                raise RuntimeError(f"tt_embeddings: {name} must be contiguous float32 [cache_size] or [cache_size, D]")
        if old_opt_state.shape != opt_state.shape:
            raise RuntimeError("tt_embeddings: old_opt_state must have opt_state's shape")
        width, sp, osp = (1 if opt_state.dim() == 1 else D), opt_state.data_ptr(), old_opt_state.data_ptr()
    if any(t.device != dev for t in (hashtbl, old_state, cache_state, ow) + (() if opt_state is None else (opt_state, old_opt_state))):
        raise RuntimeError(f"tt_embeddings: every cache_carry tensor must be on {dev}")
    with _guard(dev):
        _check(lib().ttx_cache_carry(H, hashtbl.data_ptr(), old_state.data_ptr(), cache_state.data_ptr(), cs, D, ow.data_ptr(),
                                     cw.data_ptr(), width, osp, sp, _stream(dev)))


def preprocess_indices_sync(colidx: torch.Tensor, offsets: torch.Tensor, num_tables: int, warmup: bool,
                            hashtbl: torch.Tensor, cache_state: torch.Tensor,
                            update_cache_freq: Optional[torch.Tensor] = None
                            ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, int, Optional[torch.Tensor]]:
    """tt_embeddings.cpp:88-95.  Host-synchronous iff not warmup and num_tables == 1.
    Extra (not in the reference): `update_cache_freq` folds update_cache_state(colidx, hashtbl,
    update_cache_freq) into the same launch."""
    dev = _dev(colidx)
    colidx, offsets = _i64(colidx, "colidx"), _i64(offsets, "offsets")
    nnz = colidx.numel()
    rowidx = torch.empty_like(colidx)
    tableidx = torch.empty_like(colidx)
    if nnz == 0:
        return colidx, rowidx, tableidx, 0, None
    live = (not warmup) and num_tables == 1
    pcol = prow = ploc = None
    lb = lib()
    st = _stream(dev)
    wsp, wsn = None, 0
    if live:
        pcol, prow = torch.empty_like(colidx), torch.empty_like(colidx)
        ploc = torch.empty(nnz, dtype=torch.int32, device=dev)
        ws = _workspace(dev, st, lb.ttx_preprocess_workspace_bytes(nnz))
        wsp, wsn = ws.data_ptr(), ws.numel()
    num_tt, part = C.c_int32(0), C.c_int32(0)
    fuse = update_cache_freq is not None and hashtbl.numel() > 0
    if fuse and hashtbl.numel() != update_cache_freq.numel():
        raise RuntimeError("tt_embeddings: hashtbl must match cache_freq")
    with _guard(dev):
        _check(lb.ttx_preprocess_indices_sync_fused(
            nnz, colidx.data_ptr(), offsets.numel() - 1, offsets.data_ptr(), num_tables, int(bool(warmup)),
            hashtbl.numel(), hashtbl.data_ptr() if (live or fuse) else None, cache_state.data_ptr() if live else None,
            rowidx.data_ptr(), tableidx.data_ptr(), pcol.data_ptr() if live else None,
            prow.data_ptr() if live else None, ploc.data_ptr() if live else None,
            C.byref(num_tt), C.byref(part), hashtbl.data_ptr() if fuse else None,
            update_cache_freq.data_ptr() if fuse else None, wsp, wsn, st))
    if part.value:
        return pcol, prow, tableidx, int(num_tt.value), ploc
    return colidx, rowidx, tableidx, nnz, None


def preprocess_indices_async(colidx: torch.Tensor, offsets: torch.Tensor, hashtbl: torch.Tensor, cache_state: torch.Tensor,
                             update_cache_freq: Optional[torch.Tensor] = None
                             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Not in the reference: preprocess_indices_sync of ONE table with a live cache, the split point left on the device and no
    synchronise (ttx_preprocess_indices_async).  -> (pcol, prow, ploc, n_tt_dev): the batch partitioned into misses (in front, in
    their order) and hits, the bag row of every partitioned lookup, its cache row (-1 for a miss), and the number of misses as
    one int32 on the device.  `update_cache_freq` folds update_cache_state(colidx, hashtbl, update_cache_freq) into the same
    launch, in the order "count, then look up"."""
    dev = _dev(colidx)
    colidx, offsets = _i64(colidx, "colidx"), _i64(offsets, "offsets")
    _i64(hashtbl, "hashtbl")
    nnz, H = colidx.numel(), hashtbl.numel()
    if H <= 0 or cache_state.dtype != torch.int32 or cache_state.numel() != H:
        raise RuntimeError("tt_embeddings: need a non-empty hashtbl and cache_state int32[hashtbl_size]")
    fuse = update_cache_freq is not None
    if fuse and update_cache_freq.numel() != H:
        raise RuntimeError("tt_embeddings: hashtbl must match cache_freq")
    if offsets.numel() < 1 or hashtbl.device != dev or cache_state.device != dev or offsets.device != dev:
        raise RuntimeError(f"tt_embeddings: offsets (with their closing entry), hashtbl and cache_state must be on {dev}")
    pcol, prow = torch.empty_like(colidx), torch.empty_like(colidx)
    ploc = torch.empty(nnz, dtype=torch.int32, device=dev)
    n_tt_dev = torch.empty(1, dtype=torch.int32, device=dev)
    if nnz == 0:
        return pcol, prow, ploc, n_tt_dev.zero_()
    rowidx, tableidx = torch.empty_like(colidx), torch.empty_like(colidx)
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_preprocess_workspace_bytes(nnz))
    num_tt, part = C.c_int32(0), C.c_int32(0)
    with _guard(dev):
        _check(lb.ttx_preprocess_indices_async(
            nnz, colidx.data_ptr(), offsets.numel() - 1, offsets.data_ptr(), 1, 0, H, hashtbl.data_ptr(), cache_state.data_ptr(),
            rowidx.data_ptr(), tableidx.data_ptr(), pcol.data_ptr(), prow.data_ptr(), ploc.data_ptr(), C.byref(num_tt),
            C.byref(part), n_tt_dev.data_ptr(), hashtbl.data_ptr() if fuse else None,
            update_cache_freq.data_ptr() if fuse else None, ws.data_ptr(), ws.numel(), st))
    return pcol, prow, ploc, n_tt_dev


def _check_cached_args(nnz: int, cache_locations: torch.Tensor, rowidx: torch.Tensor) -> None:
    if cache_locations.dtype != torch.int32 or not cache_locations.is_contiguous():
        raise RuntimeError("tt_embeddings: cache_locations must be contiguous int32")
    if nnz > cache_locations.numel() or nnz > rowidx.numel():
        raise RuntimeError("tt_embeddings: nnz exceeds cache_locations / rowidx")


def cache_forward(B: int, nnz: int, cache_locations: torch.Tensor, rowidx: torch.Tensor, cache_weight: torch.Tensor,
                  output: torch.Tensor, skip_dev: Optional[torch.Tensor] = None) -> None:
    """tt_embeddings.cpp:97-103: output[rowidx[n], :] += cache_weight[cache_locations[n], :].  `skip_dev` (trailing keyword, not
    in the reference): one int32 on the device, the number of LEADING entries of cache_locations / rowidx that are not cached --
    the arrays are the whole partitioned batch of `nnz` lookups and the gather works on [*skip_dev, nnz) (ttx_cache_forward_n)."""
    dev = _dev(output)
    if B <= 0:
        raise RuntimeError("tt_embeddings: B must be > 0")  # cu:1549
    if nnz == 0:
        return
    _check_cached_args(nnz, cache_locations, rowidx)
    cw = cache_weight.detach()
    if skip_dev is not None:
        with _guard(dev):
            _check(lib().ttx_cache_forward_n(B, nnz, _skip_ptr(skip_dev, dev), cache_locations.data_ptr(),
                                             _i64(rowidx, "rowidx").data_ptr(), cw.size(1), cw.data_ptr(), output.data_ptr(),
                                             _stream(dev)))
        return
    with _guard(dev):
        _check(lib().ttx_cache_forward(B, nnz, cache_locations.data_ptr(), _i64(rowidx, "rowidx").data_ptr(), cw.size(1),
                                       cw.data_ptr(), output.data_ptr(), _stream(dev)))


# The cache rows' update WITHOUT atomics (ttx_cache_backward_sorted: the cached lookups grouped by cache row with a stable sort, a
# row's bag gradients added in index order, one writer per row -- bit-identical from run to run, and the sequential oracle's order
# for row-wise Adagrad).  `deterministic` (trailing keyword of the three functions below, not in the reference): True = always,
# False = the one-launch float-atomic kernels (the reference's own formulation; the last bits of cache_weight then depend on the
# order the adds arrive in), None = "auto": sorted from DETERMINISTIC_AUTO_MIN_NNZ cached lookups on (row-wise Adagrad:
# DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD), where it is also the faster of the two.  TTX_DETERMINISTIC=1 / 0 in the environment overrides None.
# (measured, profiles/r06_cache_bandwidth.md: the sorted update is a chain of ~16 launches, ~65 us whatever the batch; on a Zipf
#  stream it overtakes the atomic SGD / dense scatter near 300k cached lookups -- 232 against 343 us at 1 M -- and the atomic
#  row-wise Adagrad, whose hot rows serialise, near 60k -- 357 against 1228 us at 1 M)
DETERMINISTIC_AUTO_MIN_NNZ = int(os.environ.get("TTX_DETERMINISTIC_AUTO_MIN_NNZ", 262144))
DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD = int(os.environ.get("TTX_DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD", 65536))


def _use_sorted(deterministic: Optional[bool], nnz: int, adagrad: bool = False) -> bool:
    if deterministic is None and os.environ.get("TTX_DETERMINISTIC", "") != "":
        deterministic = os.environ["TTX_DETERMINISTIC"] not in ("0", "")
    if deterministic is None:
        return nnz >= (DETERMINISTIC_AUTO_MIN_NNZ_ADAGRAD if adagrad else DETERMINISTIC_AUTO_MIN_NNZ)
    return bool(deterministic)


def _cache_backward_sorted(optim: int, nnz: int, go: torch.Tensor, cache_locations: torch.Tensor, rowidx: torch.Tensor, lr: float,
                           eps: float, state: Optional[torch.Tensor], dst: torch.Tensor, skip_dev: Optional[torch.Tensor] = None) -> None:
    dev = _dev(dst)
    D, cs = dst.size(1), dst.size(0)
    num_bags = go.numel() // D
    lb = lib()
    st = _stream(dev)
    nb = lb.ttx_cache_backward_sorted_workspace_bytes(nnz, num_bags, D)
    ws = _workspace(dev, st, nb)
    with _guard(dev):
        _check(lb.ttx_cache_backward_sorted(optim, nnz, None if skip_dev is None else skip_dev.data_ptr(), num_bags, D, go.data_ptr(),
                                            cache_locations.data_ptr() if nnz else None,
                                            _i64(rowidx, "rowidx").data_ptr() if nnz else None, lr, eps, cs,
                                            None if state is None else state.data_ptr(), dst.data_ptr(),
                                            ws.data_ptr() if nnz else None, ws.numel(), st))


def _skip_ptr(skip_dev: torch.Tensor, dev: torch.device) -> int:
    if skip_dev.dtype != torch.int32 or skip_dev.numel() != 1 or skip_dev.device != dev:
        raise RuntimeError(f"tt_embeddings: skip_dev must be one int32 on {dev}, got {skip_dev.dtype} x {skip_dev.numel()} on "
                           f"{skip_dev.device}")
    return skip_dev.data_ptr()


def cache_backward_sgd(nnz: int, grad_output: torch.Tensor, cache_locations: torch.Tensor, rowidx: torch.Tensor,
                       learning_rate: float, cache_weight: torch.Tensor, deterministic: Optional[bool] = None,
                       skip_dev: Optional[torch.Tensor] = None) -> None:
    """tt_embeddings.cpp:105-111.  `skip_dev` (trailing keyword of the three functions below, not in the reference): one int32 on
    the device, the number of LEADING entries of cache_locations / rowidx that are not cached -- the arrays are the whole
    partitioned batch of `nnz` lookups and the update works on [*skip_dev, nnz): no host read-back of the split point
    (ttx_cache_backward_*_n; `deterministic=None` then looks at nnz, the batch)."""
    if nnz == 0:
        return
    dev = _dev(cache_weight)
    cw = cache_weight.detach()
    go = _f32(grad_output, "grad_output")
    _check_cached_args(nnz, cache_locations, rowidx)
    if _use_sorted(deterministic, nnz):
        return _cache_backward_sorted(OPTIM_SGD, nnz, go, cache_locations, rowidx, learning_rate, 0.0, None, cw, skip_dev)
    if skip_dev is not None:
        with _guard(dev):
            _check(lib().ttx_cache_backward_sgd_n(nnz, _skip_ptr(skip_dev, dev), cw.size(1), go.data_ptr(), cache_locations.data_ptr(),
                                                  _i64(rowidx, "rowidx").data_ptr(), learning_rate, cw.data_ptr(), _stream(dev)))
        return
    with _guard(dev):
        _check(lib().ttx_cache_backward_sgd(nnz, cw.size(1), go.data_ptr(), cache_locations.data_ptr(),
                                            _i64(rowidx, "rowidx").data_ptr(), learning_rate, cw.data_ptr(), _stream(dev)))


def cache_backward_dense(nnz: int, grad_output: torch.Tensor, cache_locations: torch.Tensor, rowidx: torch.Tensor,
                         learning_rate: float, cache_weight: torch.Tensor, deterministic: Optional[bool] = None,
                         skip_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tt_embeddings.cpp:113-119 (learning_rate unused, as in the reference)."""
    dev = _dev(cache_weight)
    cw = cache_weight.detach()
    out = torch.empty_like(cw)
    go = _f32(grad_output, "grad_output")
    _check_cached_args(nnz, cache_locations, rowidx)
    if _use_sorted(deterministic, nnz):
        _cache_backward_sorted(OPTIM_DENSE, nnz, go, cache_locations, rowidx, 0.0, 0.0, None, out, skip_dev)
        return out
    if skip_dev is not None:
        with _guard(dev):
            _check(lib().ttx_cache_backward_dense_n(nnz, _skip_ptr(skip_dev, dev), cw.size(1), go.data_ptr(),
                                                    cache_locations.data_ptr() if nnz else None,
                                                    _i64(rowidx, "rowidx").data_ptr() if nnz else None, cw.size(0),
                                                    out.data_ptr(), _stream(dev)))
        return out
    with _guard(dev):
        _check(lib().ttx_cache_backward_dense(nnz, cw.size(1), go.data_ptr(),
                                              cache_locations.data_ptr() if nnz else None,
                                              _i64(rowidx, "rowidx").data_ptr() if nnz else None, cw.size(0),
                                              out.data_ptr(), _stream(dev)))
    return out


def cache_backward_rowwise_adagrad_approx(nnz: int, grad_output: torch.Tensor, cache_locations: torch.Tensor,
                                          rowidx: torch.Tensor, learning_rate: float, eps: float,
                                          cache_optimizer_state: torch.Tensor, cache_weight: torch.Tensor,
                                          deterministic: Optional[bool] = None,
                                          skip_dev: Optional[torch.Tensor] = None) -> None:
    """tt_embeddings.cpp:121-129."""
    if nnz == 0:
        return
    dev = _dev(cache_weight)
    cw = cache_weight.detach()
    go = _f32(grad_output, "grad_output")
    _dev(cache_optimizer_state)
    _check_cached_args(nnz, cache_locations, rowidx)
    if _use_sorted(deterministic, nnz, adagrad=True):
        return _cache_backward_sorted(OPTIM_ADAGRAD, nnz, go, cache_locations, rowidx, learning_rate, eps, cache_optimizer_state, cw,
                                      skip_dev)
    if skip_dev is not None:
        with _guard(dev):
            _check(lib().ttx_cache_backward_rowwise_adagrad_approx_n(
                nnz, _skip_ptr(skip_dev, dev), cw.size(1), go.data_ptr(), cache_locations.data_ptr(), _i64(rowidx, "rowidx").data_ptr(),
                learning_rate, eps, cache_optimizer_state.data_ptr(), cw.data_ptr(), _stream(dev)))
        return
    with _guard(dev):
        _check(lib().ttx_cache_backward_rowwise_adagrad_approx(
            nnz, cw.size(1), go.data_ptr(), cache_locations.data_ptr(), _i64(rowidx, "rowidx").data_ptr(),
            learning_rate, eps, cache_optimizer_state.data_ptr(), cw.data_ptr(), _stream(dev)))


# --------------------------------------------------------------------------- #
# extras
# --------------------------------------------------------------------------- #

def tt_rows(num_tables, D, tt_p_shapes, tt_q_shapes, tt_ranks, indices, tableidx, tt_cores) -> torch.Tensor:
    """Decompress rows: rows[n, :] = TT row of indices[n] (contraction only)."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(tt_cores[0])
    cores = _cores(tt_cores, g)
    indices = _i64(indices, "indices")
    nnz = indices.numel()
    rows = torch.empty((nnz, D), dtype=torch.float32, device=dev)
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_plan_bytes(C.byref(g), nnz) + 256)
    with _guard(dev):
        _check(lb.ttx_tt_rows(C.byref(g), D, nnz, indices.data_ptr(),
                              None if tableidx is None else _i64(tableidx, "tableidx").data_ptr(), _ptr_array(cores),
                              rows.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return rows


# ---- pooling modes: nn.EmbeddingBag(mode="mean" / "max") (include/ttx.h "pooling modes") ----
def bag_mean_scale(x: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """y[b, :] = x[b, :] / max(1, bag length) for x [..., D] holding nb = offsets.numel() - 1 rows (a new tensor)."""
    dev = _dev(x)
    x = _f32(x, "x")
    offsets = _i64(offsets, "offsets")
    nb, D = offsets.numel() - 1, x.size(-1)
    if x.numel() != nb * D:
        raise RuntimeError(f"tt_embeddings: bag_mean_scale needs {nb} rows of {D}, got {tuple(x.shape)}")
    y = torch.empty_like(x)
    with _guard(dev):
        _check(lib().ttx_bag_mean_scale(nb, D, offsets.data_ptr(), x.data_ptr(), y.data_ptr(), _stream(dev)))
    return y


def tt_rows_p(num_tables, D, tt_p_shapes, tt_q_shapes, tt_ranks, indices, tableidx, tt_cores,
              plan: Optional[Plan] = None) -> torch.Tensor:
    """tt_rows with the batch's plan (make_plan(..., rowidx=None)): rows [nnz, D]; the plan then serves tt_backward_rows."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(tt_cores[0])
    cores = _cores(tt_cores, g)
    indices, tableidx = _i64(indices, "indices"), _i64(tableidx, "tableidx")
    nnz = indices.numel()
    rows = torch.empty((nnz, D), dtype=torch.float32, device=dev)
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, 0 if plan is not None else lb.ttx_plan_bytes(C.byref(g), nnz) + 256)
    with _guard(dev):
        _check(lb.ttx_tt_rows_p(C.byref(g), D, nnz, indices.data_ptr(), tableidx.data_ptr(), _ptr_array(cores), rows.data_ptr(),
                                _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
    return rows


# ---- bf16 inference forward (include/ttx.h "bf16 inference forward"; the module on top: ttx_infer.TTInferenceBag) ----
def tt_rows_bf16_supported(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks) -> bool:
    """does the bf16 rows kernel take this geometry (T = 3, ranks <= 64, ...)?  Host-side: no GPU needed."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    return bool(lib().ttx_tt_rows_bf16_supported(C.byref(g)))


def pack_cores_bf16(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, tt_cores) -> List[torch.Tensor]:
    """the fp32 cores rounded to bf16 (nearest even, as tensor.to(torch.bfloat16)) in the packed layout of the bf16 rows
    kernel: one flat bfloat16 tensor per core."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(tt_cores[0])
    cores = _cores(tt_cores, g)
    lb = lib()
    out = []
    with _guard(dev):
        for t, c in enumerate(cores):
            n = lb.ttx_tt_pack_bf16_elems(C.byref(g), t)
            if n <= 0:
                raise RuntimeError("tt_embeddings: pack_cores_bf16: the bf16 kernel does not take this geometry "
                                   "(tt_rows_bf16_supported)")
            pk = torch.empty(n, dtype=torch.bfloat16, device=dev)
            _check(lb.ttx_tt_pack_bf16(C.byref(g), t, c.data_ptr(), pk.data_ptr(), _stream(dev)))
            out.append(pk)
    return out


def tt_rows_bf16(num_tables, D, tt_p_shapes, tt_q_shapes, tt_ranks, indices, tableidx, packed_cores,
                 plan: Optional[Plan] = None) -> torch.Tensor:
    """rows [nnz, D] float32 in lookup order from the packed bf16 cores of pack_cores_bf16; `plan`: the batch's plan
    (make_plan / lookup_prologue), None: built in the workspace."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    dev = _dev(packed_cores[0])
    if len(packed_cores) != 3 or any(c.dtype != torch.bfloat16 or not c.is_contiguous() or c.device != dev for c in packed_cores):
        raise RuntimeError("tt_embeddings: tt_rows_bf16 needs the three packed bfloat16 cores of pack_cores_bf16 on one device")
    lb = lib()
    for t, c in enumerate(packed_cores):
        if c.numel() != lb.ttx_tt_pack_bf16_elems(C.byref(g), t):
            raise RuntimeError(f"tt_embeddings: packed core {t} holds {c.numel()} elements, the geometry needs "
                               f"{lb.ttx_tt_pack_bf16_elems(C.byref(g), t)}")
    indices = _i64(indices, "indices")
    nnz = indices.numel()
    rows = torch.empty((nnz, D), dtype=torch.float32, device=dev)
    st = _stream(dev)
    ws = _workspace(dev, st, 0 if plan is not None else lb.ttx_tt_rows_bf16_workspace_bytes(C.byref(g), D, nnz))
    with _guard(dev):
        _check(lb.ttx_tt_rows_bf16(C.byref(g), D, nnz, indices.data_ptr(),
                                   None if tableidx is None else _i64(tableidx, "tableidx").data_ptr(), _ptr_array(packed_cores),
                                   rows.data_ptr(), _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
    return rows


def bag_sum_pool(rows: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """-> [nb, D]: the fp32 sum of each bag's rows in index order (rows in lookup order, bags contiguous; offsets with
    their closing entry); an empty bag gives zeros."""
    dev = _dev(rows)
    rows, offsets = _f32(rows, "rows"), _i64(offsets, "offsets")
    nb, D = offsets.numel() - 1, rows.size(1)
    out = torch.empty((nb, D), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(lib().ttx_bag_sum_pool(nb, D, offsets.data_ptr(), rows.data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def bag_max_pool(rows: torch.Tensor, offsets: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (output [nb, D]: column-wise max of each bag's rows, argmax [nb, D] int32: the position of the row that holds it --
    the first one on a tie, -1 for an empty bag, whose output is 0)."""
    dev = _dev(rows)
    rows, offsets = _f32(rows, "rows"), _i64(offsets, "offsets")
    nb, D = offsets.numel() - 1, rows.size(1)
    out = torch.empty((nb, D), dtype=torch.float32, device=dev)
    arg = torch.empty((nb, D), dtype=torch.int32, device=dev)
    with _guard(dev):
        _check(lib().ttx_bag_max_pool(nb, D, rows.size(0), offsets.data_ptr(), rows.data_ptr(), out.data_ptr(), arg.data_ptr(),
                                      _stream(dev)))
    return out, arg


def bag_max_pool_backward(d_output: torch.Tensor, argmax: torch.Tensor, offsets: torch.Tensor, nnz: int) -> torch.Tensor:
    """d_rows [nnz, D]: lookup n's row carries the gradient of the columns it won in its bag, zeros elsewhere."""
    dev = _dev(d_output)
    d_output, offsets = _f32(d_output, "d_output"), _i64(offsets, "offsets")
    if argmax.dtype != torch.int32 or not argmax.is_contiguous():
        raise RuntimeError("tt_embeddings: argmax must be contiguous int32")
    nb, D = offsets.numel() - 1, argmax.size(-1)
    if d_output.numel() != nb * D or argmax.numel() != nb * D:
        raise RuntimeError(f"tt_embeddings: bag_max_pool_backward needs {nb} rows of {D}")
    d_rows = torch.empty((nnz, D), dtype=torch.float32, device=dev)
    with _guard(dev):
        _check(lib().ttx_bag_max_pool_backward(nb, D, nnz, offsets.data_ptr(), argmax.data_ptr(), d_output.data_ptr(),
                                               d_rows.data_ptr(), _stream(dev)))
    return d_rows


def tt_backward_rows(optim, D, lr, eps, p, q, ranks, nnz, indices, tableidx, d_rows, tt_cores, state=None,
                     plan: Optional[Plan] = None) -> Optional[List[torch.Tensor]]:
    """the backward with one gradient row per lookup (d_rows [nnz, D]); optim OPTIM_SGD / OPTIM_ADAGRAD update the cores (and
    the Adagrad state) in place, OPTIM_DENSE returns the core gradients.  plan: the one tt_rows_p ran on, or None."""
    g = _geom(tt_cores[0].size(0), p, q, ranks)
    dev = _dev(d_rows)
    cores = _cores(tt_cores, g)
    d_rows = _f32(d_rows, "d_rows")
    if d_rows.dim() != 2 or d_rows.size(0) != nnz or d_rows.size(1) != D:
        raise RuntimeError(f"tt_embeddings: d_rows must be [nnz, D] = [{nnz}, {D}], got {tuple(d_rows.shape)}")
    indices, tableidx = _i64(indices, "indices"), _i64(tableidx, "tableidx")
    grads = [torch.empty_like(c) for c in cores] if optim == OPTIM_DENSE else None
    sptr = _ptr_array(_cores(state, g, "optimizer_state")) if optim == OPTIM_ADAGRAD else None
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_tt_backward_rows_workspace_bytes(C.byref(g), D, nnz))
    with _guard(dev):
        _check(lb.ttx_tt_backward_rows(C.byref(g), optim, D, lr, eps, nnz, indices.data_ptr(), tableidx.data_ptr(),
                                       d_rows.data_ptr(), _ptr_array(cores), sptr, None if grads is None else _ptr_array(grads),
                                       _plan_ptr(plan, nnz), ws.data_ptr(), ws.numel(), st))
    return grads


# ---- padded bags: nn.EmbeddingBag(padding_idx=) (include/ttx.h "padded bags") ----
def bags_compact(indices: torch.Tensor, offsets: Optional[torch.Tensor], L: int, padding_idx: int
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Drop the slots that hold `padding_idx`, keeping the order of the others.  Bags: `offsets` [nb + 1] int64 with the closing
    entry, or None for indices.numel() // L bags of L slots each.  -> (out_indices [nnz]: the live slots, then zeros;
    out_offsets [nb + 1]: the bags of the live slots; n_live: one int32 on the device = out_offsets[nb]).  No host read-back."""
    dev = _dev(indices)
    indices = _i64(indices, "indices").reshape(-1)
    nnz = indices.numel()
    if offsets is not None:
        offsets = _i64(offsets, "offsets")
        nb = offsets.numel() - 1
        if nb < 0:
            raise RuntimeError("tt_embeddings: offsets must hold the closing entry")
    else:
        L = int(L)
        if L < 0 or (L == 0 and nnz != 0) or (L > 0 and nnz % L != 0):
            raise RuntimeError(f"tt_embeddings: bags_compact without offsets needs bags of L slots, got {nnz} slots for L = {L}")
        nb = nnz // L if L > 0 else 0
    out_i = torch.empty(nnz, dtype=torch.int64, device=dev)
    out_o = torch.empty(nb + 1, dtype=torch.int64, device=dev)
    n_live = torch.empty(1, dtype=torch.int32, device=dev)
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_bags_compact_workspace_bytes(nb, nnz))
    with _guard(dev):
        _check(lb.ttx_bags_compact(nb, nnz, indices.data_ptr(), None if offsets is None else offsets.data_ptr(), int(L),
                                   int(padding_idx), out_i.data_ptr(), out_o.data_ptr(), n_live.data_ptr(), ws.data_ptr(),
                                   ws.numel(), st))
    return out_i, out_o, n_live


# ---- unpooled rows at padded positions: nn.Embedding(padding_idx=) (include/ttx.h "unpooled rows at padded positions") ----
def _rank_rows(rank: torch.Tensor, x: torch.Tensor, name: str):
    dev = _dev(x)
    rank, x = _i64(rank, "rank"), _f32(x, name)
    n = rank.numel() - 1
    if rank.device != dev or n < 0 or x.dim() != 2 or x.size(0) != n:
        raise RuntimeError(f"tt_embeddings: rank must hold n + 1 entries on {dev} for {name} [n, D], got {rank.numel()} on "
                           f"{rank.device} and {tuple(x.shape)}")
    return dev, rank, x, n


def rows_expand(rank: torch.Tensor, rows: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[i, :] = rows[rank[i], :] where position i is live (rank[i + 1] > rank[i]), exact zeros elsewhere.  rank [n + 1] is
    bags_compact's out_offsets of n one-slot bags; rows / out [n, D].  Every element of `out` is written."""
    dev, rank, rows, n = _rank_rows(rank, rows, "rows")
    if out is None:
        out = torch.empty_like(rows)
    elif out.shape != rows.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"tt_embeddings: out must be a contiguous float32 {tuple(rows.shape)} on {dev}")
    with _guard(dev):
        _check(lib().ttx_rows_expand(n, rows.size(1), rank.data_ptr(), rows.data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def rows_collect(rank: torch.Tensor, d_out: torch.Tensor) -> torch.Tensor:
    """d_rows[rank[i], :] = d_out[i, :] for the live positions i: the gradient rows in compacted order.  -> d_rows [n, D], whose
    rows at and beyond rank[n] are not written (the plan's live count keeps the backward away from them)."""
    dev, rank, d_out, n = _rank_rows(rank, d_out, "d_out")
    d_rows = torch.empty_like(d_out)
    with _guard(dev):
        _check(lib().ttx_rows_collect(n, d_out.size(1), rank.data_ptr(), d_out.data_ptr(), d_rows.data_ptr(), _stream(dev)))
    return d_rows


# ---- unpooled rows with a live cache (include/ttx.h "unpooled rows with a live cache") ----
def _split_args(n: int, n_tt, dev: torch.device):
    """(host n_tt, device pointer or None) of a split point given as an int or as one int32 on the device"""
    if isinstance(n_tt, torch.Tensor):
        if n_tt.dtype != torch.int32 or n_tt.numel() != 1 or n_tt.device != dev:
            raise RuntimeError(f"tt_embeddings: n_tt must be an int or one int32 on {dev}, got {n_tt.dtype} x {n_tt.numel()} on "
                               f"{n_tt.device}")
        return n, n_tt.data_ptr()
    return int(n_tt), None


def rows_place(N: int, n_tt, pos: torch.Tensor, loc: torch.Tensor, rows_tt: torch.Tensor, cache_weight: torch.Tensor,
               rank: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[pos[s], :] = rows_tt[s, :] for the misses s < n_tt, cache_weight[loc[s], :] for the hits n_tt <= s < n = pos.numel(), and
    exact zeros at the padding positions of `rank` (bags_compact's out_offsets of N one-slot bags; None: no padding, n == N).
    pos / loc: part_rowidx / part_cache_locations of preprocess_indices_async; n_tt: its split point, one int32 on the device (or
    an int).  -> out [N, D]; every element is written."""
    dev = _dev(rows_tt)
    rows_tt, cw = _f32(rows_tt, "rows_tt"), _f32(cache_weight.detach(), "cache_weight")
    pos = _i64(pos, "pos")
    n, D = pos.numel(), cw.size(1)
    if loc.dtype != torch.int32 or not loc.is_contiguous() or loc.numel() < n:
        raise RuntimeError("tt_embeddings: loc must be contiguous int32, one entry per partitioned lookup")
    if rows_tt.dim() != 2 or rows_tt.size(1) != D or rows_tt.size(0) < n or cw.dim() != 2:
        raise RuntimeError(f"tt_embeddings: rows_tt must be [>= {n}, {D}] beside cache_weight [cache_size, {D}], got {tuple(rows_tt.shape)}")
    if any(t.device != dev for t in (pos, loc, cw)) or (rank is not None and rank.device != dev):
        raise RuntimeError(f"tt_embeddings: pos, loc, cache_weight and rank must be on {dev}")
    if rank is not None:
        rank = _i64(rank, "rank")
        if rank.numel() != N + 1:
            raise RuntimeError(f"tt_embeddings: rank must hold N + 1 = {N + 1} entries, got {rank.numel()}")
    if out is None:
        out = torch.empty((N, D), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (N, D) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != dev:
        raise RuntimeError(f"tt_embeddings: out must be a contiguous float32 {(N, D)} on {dev}")
    n_tt_host, n_tt_ptr = _split_args(n, n_tt, dev)
    with _guard(dev):
        _check(lib().ttx_rows_place(N, n, n_tt_host, n_tt_ptr, D, pos.data_ptr(), loc.data_ptr(), rows_tt.data_ptr(), cw.data_ptr(),
                                    cw.size(0), None if rank is None else rank.data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def rows_pick(n_tt, pos: torch.Tensor, d_out: torch.Tensor) -> torch.Tensor:
    """d_rows[s, :] = d_out[pos[s], :] for the misses s < n_tt: their gradient rows in partition order.  d_out [N, D]
    -> d_rows [N, D], whose rows at and beyond n_tt are not written (the plan's count keeps the backward away from them)."""
    dev = _dev(d_out)
    d_out, pos = _f32(d_out, "d_out"), _i64(pos, "pos")
    if d_out.dim() != 2 or pos.device != dev or pos.numel() > d_out.size(0):
        raise RuntimeError(f"tt_embeddings: d_out must be [N, D] on the device of pos with N >= pos.numel(), got {tuple(d_out.shape)}")
    N, D, n = d_out.size(0), d_out.size(1), pos.numel()
    d_rows = torch.empty_like(d_out)
    n_tt_host, n_tt_ptr = _split_args(n, n_tt, dev)
    with _guard(dev):
        _check(lib().ttx_rows_pick(N, n, n_tt_host, n_tt_ptr, D, pos.data_ptr(), d_out.data_ptr(), d_rows.data_ptr(), _stream(dev)))
    return d_rows


# ---- merged bags: per-table batches -> one table-major batch (include/ttx.h "merged bags") ----
_WIDTH = {torch.int64: 8, torch.int32: 4}


def bags_merge(indices: Sequence[torch.Tensor], offsets: Sequence[Optional[torch.Tensor]], include_last_offset: bool,
               per_sample_weights: Optional[Sequence[Optional[torch.Tensor]]] = None,
               padding: Optional[Sequence[Optional[int]]] = None, sentinel: int = -1
               ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """One batch per table -> the table-major batch of a table-batched lookup, in one launch (64 tables per launch).  Table k:
    `indices[k]` int64 / int32, 1-D with `offsets[k]` (B bag starts, plus the closing entry when `include_last_offset`), or 2-D
    [B, L_k] with `offsets[k] = None`; `per_sample_weights[k]` float32 of the shape of indices[k], or None for ones;
    `padding[k]`: slots that hold it are written as `sentinel`.  -> (out_indices [N] int64, out_offsets [ntab * B + 1] int64,
    out_weights [N] float32 -- None unless some table has weights).  No host read-back."""
    ntab = len(indices)
    if ntab < 1 or len(offsets) != ntab:
        raise RuntimeError(f"tt_embeddings: bags_merge needs one (indices, offsets) pair per table, got {ntab} and {len(offsets)}")
    if per_sample_weights is not None and all(w is None for w in per_sample_weights):
        per_sample_weights = None
    for name, seq in (("per_sample_weights", per_sample_weights), ("padding", padding)):
        if seq is not None and len(seq) != ntab:
            raise RuntimeError(f"tt_embeddings: bags_merge: {name} must have one entry per table")
    dev = _dev(indices[0])
    # (plain lists first, one ctypes array each at the end: this loop is host time in front of every step of a host-bound module)
    width = _WIDTH
    p_idx, p_off, p_w, v_nnz, v_L, v_pad, v_ib, v_ob, v_has = [], [], [], [], [], [], [], [], []
    keep, B = [], None
    drop = 1 if include_last_offset else 0
    for k in range(ntab):
        idx, off = indices[k], offsets[k]
        ib = width.get(idx.dtype)
        if ib is None or idx.device != dev:
            raise RuntimeError(f"tt_embeddings: bags_merge: indices[{k}] must be int64 or int32 on {dev}, got {idx.dtype} on {idx.device}")
        if not idx.is_contiguous():
            idx = idx.contiguous()
            keep.append(idx)
        if off is None:
            if idx.dim() != 2:
                raise RuntimeError(f"tt_embeddings: bags_merge: indices[{k}] without offsets must be 2-D [B, L]")
            nb, L = idx.shape
            p_off.append(0)
            v_ob.append(8)
        else:
            ob = width.get(off.dtype)
            if idx.dim() != 1 or off.dim() != 1:
                raise RuntimeError(f"tt_embeddings: bags_merge: indices[{k}] and offsets[{k}] must be 1-D")
            if ob is None or off.device != dev:
                raise RuntimeError(f"tt_embeddings: bags_merge: offsets[{k}] must be int64 or int32 on {dev}, got {off.dtype} on {off.device}")
            if not off.is_contiguous():
                off = off.contiguous()
                keep.append(off)
            nb, L = off.numel() - drop, 0
            p_off.append(off.data_ptr())
            v_ob.append(ob)
        if B is None:
            B = nb
        if nb != B or nb < 0:
            raise RuntimeError(f"tt_embeddings: bags_merge: every table must describe the same number of bags, got {B} and {nb}")
        if per_sample_weights is not None:
            w = per_sample_weights[k]
            if w is None:
                p_w.append(0)
            else:
                if w.device != dev or w.dtype != torch.float32 or w.shape != indices[k].shape:
                    raise RuntimeError(f"tt_embeddings: bags_merge: per_sample_weights[{k}] must be float32 on {dev} with the shape "
                                       f"of indices[{k}], got {w.dtype} {tuple(w.shape)} on {w.device}")
                w = w.detach()
                if not w.is_contiguous():
                    w = w.contiguous()
                keep.append(w)
                p_w.append(w.data_ptr())
        p_idx.append(idx.data_ptr())
        v_nnz.append(idx.numel())
        v_ib.append(ib)
        v_L.append(L)
        if padding is not None:
            v = padding[k]
            v_pad.append(0 if v is None else int(v))
            v_has.append(0 if v is None else 1)
    # (the host arrays as packed bytes: a ctypes array costs 4 us to build, there would be nine)
    q, i = struct.Struct(f"{ntab}q").pack, struct.Struct(f"{ntab}i").pack
    a_idx, a_off, a_nnz, a_L, a_ib, a_ob = q(*p_idx), q(*p_off), q(*v_nnz), q(*v_L), i(*v_ib), i(*v_ob)
    a_w = q(*p_w) if per_sample_weights is not None else None
    a_pad, a_has = (q(*v_pad), bytes(v_has)) if padding is not None else (None, None)
    N = sum(v_nnz)
    out_i = torch.empty(N, dtype=torch.int64, device=dev)
    out_o = torch.empty(ntab * B + 1, dtype=torch.int64, device=dev)
    out_w = torch.empty(N, dtype=torch.float32, device=dev) if per_sample_weights is not None else None
    with _guard(dev):
        _check(lib().ttx_bags_merge(ntab, B, drop, a_idx, a_nnz, a_ib, a_off, a_ob, a_L, a_w, a_pad, a_has, int(sentinel),
                                    out_i.data_ptr(), out_o.data_ptr(), None if out_w is None else out_w.data_ptr(), _stream(dev)))
    return out_i, out_o, out_w


# ---- dense member tables: bags over uncompressed rows (include/ttx.h "dense member tables"; csrc/ttx_dense.hip) ----
DENSE_MODES = {"sum": 0, "mean": 1, "max": 2}


def _dense_tabs(row_base: Sequence[int], padding: Optional[Sequence[Optional[int]]]):
    """the host arrays of the dense calls as packed bytes: row_base (num_tables + 1 int64), padding (-1: none) or None"""
    ntab = len(row_base) - 1
    a_base = struct.pack(f"{ntab + 1}q", *[int(v) for v in row_base])
    a_pad = None
    if padding is not None and any(v is not None for v in padding):
        if len(padding) != ntab:
            raise RuntimeError(f"tt_embeddings: dense bags: padding must have one entry per table ({ntab})")
        a_pad = struct.pack(f"{ntab}q", *[-1 if v is None else int(v) for v in padding])
    return ntab, a_base, a_pad


def _dense_batch(indices, offsets, weight, ntab):
    dev = _dev(weight)
    if weight.dtype != torch.float32 or weight.dim() != 2 or not weight.is_contiguous():
        raise RuntimeError("tt_embeddings: dense bags: weight must be contiguous float32 [R, D]")
    indices, offsets = _i64(indices, "indices"), _i64(offsets, "offsets")
    if indices.device != dev or offsets.device != dev:
        raise RuntimeError(f"tt_embeddings: dense bags: indices and offsets must live on {dev}")
    nb = offsets.numel() - 1
    if nb < 0 or nb % ntab:
        raise RuntimeError(f"tt_embeddings: dense bags: offsets needs num_tables * B + 1 entries ({ntab} tables), got {offsets.numel()}")
    return dev, indices, offsets, nb // ntab


def dense_bags_forward(indices: torch.Tensor, offsets: torch.Tensor, row_base: Sequence[int], weight: torch.Tensor,
                       mode: str = "sum", padding: Optional[Sequence[Optional[int]]] = None,
                       per_sample_weights: Optional[torch.Tensor] = None
                       ) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Bags over uncompressed tables, table-major (bag b belongs to table b // B): weight [R, D] holds table k's rows at
    [row_base[k], row_base[k + 1]).  -> (output [num_tables * B, D], live int32 per bag -- mean only, else None --, argmax int32
    [num_tables * B, D] -- max only, else None).  A negative index and `padding[table]` are padding; other indices are clamped."""
    ntab, a_base, a_pad = _dense_tabs(row_base, padding)
    dev, indices, offsets, B = _dense_batch(indices, offsets, weight, ntab)
    D, nnz, m = weight.size(1), indices.numel(), DENSE_MODES[mode]
    psw = None if per_sample_weights is None else _f32(per_sample_weights.detach(), "per_sample_weights").reshape(-1)
    if psw is not None and psw.numel() != nnz:
        raise RuntimeError("tt_embeddings: dense bags: per_sample_weights must have one entry per index")
    out = torch.empty((ntab * B, D), dtype=torch.float32, device=dev)
    live = torch.empty(ntab * B, dtype=torch.int32, device=dev) if m == 1 else None
    arg = torch.empty((ntab * B, D), dtype=torch.int32, device=dev) if m == 2 else None
    with _guard(dev):
        _check(lib().ttx_dense_bags_forward(ntab, B, D, nnz, indices.data_ptr(), offsets.data_ptr(), a_base, a_pad,
                                            None if psw is None else psw.data_ptr(), m, weight.data_ptr(), out.data_ptr(),
                                            None if live is None else live.data_ptr(), None if arg is None else arg.data_ptr(),
                                            _stream(dev)))
    return out, live, arg


def dense_bags_backward(optim: int, indices: torch.Tensor, offsets: torch.Tensor, row_base: Sequence[int], weight: torch.Tensor,
                        grad_output: torch.Tensor, mode: str = "sum", padding: Optional[Sequence[Optional[int]]] = None,
                        per_sample_weights: Optional[torch.Tensor] = None, live: Optional[torch.Tensor] = None,
                        argmax: Optional[torch.Tensor] = None, lr: float = 0.0, eps: float = 0.0,
                        opt_state: Optional[torch.Tensor] = None, want_d_psw: bool = False
                        ) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """The backward of dense_bags_forward, one update per touched row, no atomics.  optim OPTIM_SGD / OPTIM_ADAGRAD update `weight`
    (and `opt_state`: [R, D] element-wise, [R] row-wise) in place; OPTIM_DENSE returns the gradient [R, D].  -> (d_weight or None,
    d_per_sample_weights [nnz] from the weights before the update, or None unless `want_d_psw`)."""
    ntab, a_base, a_pad = _dense_tabs(row_base, padding)
    dev, indices, offsets, B = _dense_batch(indices, offsets, weight, ntab)
    D, nnz, m = weight.size(1), indices.numel(), DENSE_MODES[mode]
    grad_output = _f32(grad_output, "grad_output")
    if grad_output.numel() != ntab * B * D:
        raise RuntimeError(f"tt_embeddings: dense bags: grad_output must hold [{ntab * B}, {D}], got {tuple(grad_output.shape)}")
    psw = None if per_sample_weights is None else _f32(per_sample_weights.detach(), "per_sample_weights").reshape(-1)
    width = 0
    if optim == OPTIM_ADAGRAD:
        if opt_state is None or opt_state.dtype != torch.float32 or not opt_state.is_contiguous() or \
                opt_state.numel() not in (weight.size(0), weight.numel()):
            raise RuntimeError("tt_embeddings: dense bags: Adagrad needs a contiguous float32 opt_state of [R] or [R, D]")
        width = D if opt_state.numel() == weight.numel() else 1
    d_w = torch.empty_like(weight) if optim == OPTIM_DENSE else None
    d_psw = torch.empty(nnz, dtype=torch.float32, device=dev) if want_d_psw else None
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_dense_bags_backward_workspace_bytes(ntab * B, nnz, D))
    with _guard(dev):
        _check(lb.ttx_dense_bags_backward(optim, ntab, B, D, nnz, indices.data_ptr(), offsets.data_ptr(), a_base, a_pad,
                                          None if psw is None else psw.data_ptr(), m,
                                          None if live is None else live.data_ptr(), None if argmax is None else argmax.data_ptr(),
                                          grad_output.data_ptr(), lr, eps, width,
                                          opt_state.data_ptr() if width else None, weight.data_ptr(),
                                          None if d_w is None else d_w.data_ptr(), None if d_psw is None else d_psw.data_ptr(),
                                          ws.data_ptr(), ws.numel(), st))
    return d_w, d_psw


def dense_bags_info(D: int, nnz: int) -> dict:
    """host-side query: the sizes at which the dense backward switches behaviour -- `split`: a row with more lookups than this has
    its list summed in chunks of this length; `one_launch`: the batch size at which a one-launch route hands over (0: none)"""
    out = (C.c_int32 * 2)()
    _check(lib().ttx_dense_bags_info(int(D), int(nnz), out))
    return {"split": int(out[0]), "one_launch": int(out[1])}


# ---- fused Adam over a list of dense tensors (include/ttx.h "fused Adam"; csrc/ttx_adam.hip) ----
ADAM_MAX_TENSORS = 16


def adam_apply(weights: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], exp_avg: Sequence[torch.Tensor],
               exp_avg_sq: Sequence[torch.Tensor], step: torch.Tensor, lr: float, betas: Tuple[float, float], eps: float,
               weight_decay: float = 0.0, decoupled: bool = False) -> None:
    """One torch.optim.Adam (decoupled: AdamW) step, in place, on up to 16 float32 GPU tensors: `weights[k]`, `exp_avg[k]` and
    `exp_avg_sq[k]` are updated from `grads[k]` (same number of elements, each dense in memory -- a view offset into a buffer is
    fine), `step` (int64 [1] on the device: steps taken so far) is advanced by one.  Nothing is read back: capturable.  With no
    tensor, or elements, nothing is launched and `step` stays."""
    n = len(weights)
    if not (len(grads) == len(exp_avg) == len(exp_avg_sq) == n):
        raise RuntimeError("tt_embeddings: adam_apply: weights, grads, exp_avg and exp_avg_sq must have one entry per tensor")
    if n > ADAM_MAX_TENSORS:
        raise RuntimeError(f"tt_embeddings: adam_apply: at most {ADAM_MAX_TENSORS} tensors per call, got {n}")
    dev = _dev(step)
    if step.dtype != torch.int64 or step.numel() != 1:
        raise RuntimeError("tt_embeddings: adam_apply: step must be one int64 on the device")
    keep = []
    for k in range(n):
        w = weights[k].detach() if weights[k].requires_grad else weights[k]
        four = (w, grads[k], exp_avg[k], exp_avg_sq[k])
        for name, t in zip(("weights", "grads", "exp_avg", "exp_avg_sq"), four):
            if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.device != dev or t.numel() != w.numel():
                raise RuntimeError(f"tt_embeddings: adam_apply: {name}[{k}] must be a contiguous float32 tensor on {dev} of "
                                   f"{w.numel()} elements, got {tuple(t.shape)} {t.dtype} on {t.device}")
        keep.append(four)
    numel = (C.c_int64 * max(n, 1))(*[f[0].numel() for f in keep])
    ptrs = [_ptr_array([f[j] for f in keep]) for j in range(4)]
    lb = lib()
    st = _stream(dev)
    ws = _workspace(dev, st, lb.ttx_adam_apply_workspace_bytes(n))
    with _guard(dev):
        _check(lb.ttx_adam_apply(n, numel, ptrs[0], ptrs[1], ptrs[2], ptrs[3], step.data_ptr(), float(lr), float(betas[0]),
                                 float(betas[1]), float(eps), float(weight_decay), 1 if decoupled else 0, ws.data_ptr(), ws.numel(),
                                 st))


def profile_enable(mask: int) -> None:
    """bit w of `mask` turns on live HIP-event timing of kernel slot w (PROF_*); 0 = off."""
    _check(lib().ttx_profile_enable(int(mask)))


def profile_mask(mask: int) -> None:
    """profile_enable without draining: use around a hipGraph capture, read after the replays."""
    _check(lib().ttx_profile_mask(int(mask)))


def profile_reset() -> None:
    _check(lib().ttx_profile_reset())


def profile_read(which: int) -> Tuple[int, float]:
    n, ms = C.c_int64(0), C.c_double(0.0)
    _check(lib().ttx_profile_read(which, C.byref(n), C.byref(ms)))
    return int(n.value), float(ms.value)


def debug_sort_pairs_desc(keys: torch.Tensor, vals: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """test hook: cache_populate's stable descending 64-bit radix sort of (key, value) pairs on its own"""
    keys, vals = _i64(keys, "keys"), _i64(vals, "vals")
    dev = _dev(keys)
    n = keys.numel()
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    lb = lib()
    lb.ttx_debug_sort_workspace_bytes.restype = C.c_size_t
    lb.ttx_debug_sort_workspace_bytes.argtypes = [C.c_int64]
    lb.ttx_debug_sort_pairs_desc.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_size_t, C.c_void_p]
    nb = lb.ttx_debug_sort_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    with _guard(dev):
        _check(lb.ttx_debug_sort_pairs_desc(n, keys.data_ptr(), vals.data_ptr(), ko.data_ptr(), vo.data_ptr(), ws.data_ptr(), nb,
                                            _stream(dev)))
    return ko, vo


# ---- test / ablation knobs: libttx_hooks.so (the product library has none) ----
def set_chunk(mc: int) -> None:
    """indices per work-group chunk (0 = heuristic)"""
    _check(hooks_lib().ttx_set_chunk(int(mc)))
    _knobs_changed()


def debug_lds_budget(nbytes: int) -> None:
    """LDS budget of the generic kernels' tile search (0 = the hardware's 160 KiB)."""
    _check(hooks_lib().ttx_debug_lds_budget(int(nbytes)))
    _knobs_changed()


def debug_skip(mask: int) -> None:
    """bit 8: force the generic kernels; bit 15: exact-shape templates only; bit 16: reduce_apply with a work-group (not a wave) per
    small slice; bit 17: plans list the pivot's chunks in slot order (one column) instead of dealing them over 8 columns, one per
    XCD; bit 18: the shape-specialised backward stores its partial gradients as 4-byte non-temporal stores, as before the 16-byte
    ones; bits 19..20: the flavour of the 16-byte partial stores forced for every launch (1 non-temporal, 2 write-through, 3 plain);
    bit 21: reduce_apply_kernel also for the small launches reduce_apply_small_kernel takes
    -- these leave the results valid; the other bits skip kernel phases / launches (results INVALID).  0 = normal operation."""
    _check(hooks_lib().ttx_debug_skip(int(mask)))
    _knobs_changed()


def debug_cache_fwd(lookup_groups: int) -> None:
    _check(hooks_lib().ttx_debug_cache_fwd(int(lookup_groups)))
    _knobs_changed()


def debug_stamps(ptr: Optional[int]) -> None:
    _check(hooks_lib().ttx_debug_stamps(C.c_void_p(ptr or None)))
    _knobs_changed()


class test_library:
    """`with test_library():` -- every call of the block goes to libttx_hooks.so whatever the knobs say (the plan tests: the
    route id of debug_plan_route() belongs to the library that built the plan); afterwards the usual routing applies again."""

    def __enter__(self):
        hooks_lib()
        return _hooks

    def __exit__(self, *a):
        global _lib
        _lib = _hooks if _hooks.ttx_debug_state() else _product


PLAN_ARRAYS = ("hdr", "chunk_rec", "lrec", "lrow", "chunk_off", "cnt")
PLAN_CORE_ARRAYS = ("sid", "perm", "ipos", "off", "scratch0", "scratch1", "scratch2")


def debug_plan_layout(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks, nnz) -> dict:
    """Test helper (ttx_debug_plan_layout): {array: (offset, length) in int32 units of Plan.buf} for PLAN_ARRAYS and, per core t,
    (name, t) for PLAN_CORE_ARRAYS; plus "MC", "max_chunks", "T", "bytes"."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    out = (C.c_int64 * 72)()
    _check(hooks_lib().ttx_debug_plan_layout(C.byref(g), int(nnz), out))
    _knobs_changed()
    v = [int(x) for x in out]
    lay = {name: (v[2 * k], v[2 * k + 1]) for k, name in enumerate(PLAN_ARRAYS)}
    lay.update(MC=v[68], max_chunks=v[69], T=v[70], bytes=v[71])
    for t in range(lay["T"]):
        for j, name in enumerate(PLAN_CORE_ARRAYS):
            k = len(PLAN_ARRAYS) + len(PLAN_CORE_ARRAYS) * t + j
            lay[(name, t)] = (v[2 * k], v[2 * k + 1])
    return lay


def debug_plan_route() -> int:
    """Test helper (ttx_debug_plan_route): the route id of the last plan the TEST library built (include/ttx_test_hooks.h
    TTX_ROUTE_*; 0: none yet).  Build the plan inside `with test_library():`."""
    if _hooks is None:
        hooks_lib()
        _knobs_changed()
    return int(_hooks.ttx_debug_plan_route())


def debug_reduce_route() -> int:
    """Test helper (ttx_debug_reduce_route, a global of the TEST library): the kernel its last reduce + apply launch was --
    0 none yet, 1 reduce_apply_kernel, 2 reduce_apply_small_kernel.  Run the backward inside `with test_library():`."""
    if _hooks is None:
        hooks_lib()
        _knobs_changed()
    return int(C.c_int.in_dll(_hooks, "ttx_debug_reduce_route").value)


T4_ROUTE_FIELDS = ("merge_form", "merge_seg", "merge_grid", "seg", "helper", "lds_bytes", "lds_opt_in", "apply_seg", "q3")


def debug_t4_route(clear: bool = False) -> dict:
    """Test helper (ttx_debug_t4_route, a global of the TEST library): what the host code of the four-core route chose for its
    last launch (include/ttx_test_hooks.h TTX_T4_*; zeros: none yet).  Run the launch inside `with test_library():`.
    clear: zero the record after reading it, so that the next read shows the next launch alone."""
    if _hooks is None:
        hooks_lib()
        _knobs_changed()
    rec = (C.c_int * len(T4_ROUTE_FIELDS)).in_dll(_hooks, "ttx_debug_t4_route")
    out = dict(zip(T4_ROUTE_FIELDS, (int(x) for x in rec)))
    if clear:
        rec[:] = [0] * len(T4_ROUTE_FIELDS)
    return out


DD_ROUTE_FIELDS = ("form", "bpw", "passes", "nblk", "tstart", "pool", "gsum")


def debug_dd_route(clear: bool = False) -> dict:
    """Test helper (ttx_debug_dd_route, a global of the TEST library): what the host code of the duplicate-lookup route chose last
    (include/ttx_test_hooks.h TTX_DD_*; zeros: none yet) -- the map's form, template argument, passes and blocks and whether
    tstart was written (ttx_dedup_build), the pooling kernel (ttx_tt_forward_dd), the pre-sum's vector type (ttx_tt_backward_dd).
    Run the calls inside `with test_library():`.  clear: zero the record after reading it."""
    if _hooks is None:
        hooks_lib()
        _knobs_changed()
    rec = (C.c_int * len(DD_ROUTE_FIELDS)).in_dll(_hooks, "ttx_debug_dd_route")
    out = dict(zip(DD_ROUTE_FIELDS, (int(x) for x in rec)))
    if clear:
        rec[:] = [0] * len(DD_ROUTE_FIELDS)
    return out


def debug_tiles(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks) -> dict:
    """Test helper: the block walk the generic kernels take for this geometry under the current budget."""
    g = _geom(num_tables, tt_p_shapes, tt_q_shapes, tt_ranks)
    out = (C.c_int32 * 6)()
    _check(lib().ttx_debug_tiles(C.byref(g), out))
    return dict(zip(("MC", "bpp", "KB", "ncp", "nkb", "bytes"), [int(x) for x in out]))
