"""The bf16 inference forward (ttx_infer.TTInferenceBag) on an MI355X.

  rows     `tt_rows_bf16` (packed bf16 cores, bf16 MFMA) against `tt_rows_p` (the fp32 rows kernel) on the SAME plan, as a captured
           graph of CALLS calls replayed: device microseconds per call between two HIP events, and the bytes the call moves by
           its shapes (the cores' slices touched once, the rows written)
  forward  the whole TTInferenceBag forward against the source module's own forward under torch.no_grad(), eager and captured
  error    max |bf16 rows - fp32 rows| / max |fp32 rows|: what the rounding of the cores costs

Shapes: cfg2 (one table, 10,240 lookups, q [4,4,4], ranks 32), cfg4 (q [4,4,8], ranks 64) and cfg5's per-GPU shard (4 tables,
327,680 lookups).  The variants alternate in one process after a warm-up; medians of the windows with their min and max.

    python scripts/bench_bf16_forward.py [--windows 7] [--steps 50]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
import tt_embeddings as E  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_infer  # noqa: E402

dev = torch.device("cuda:0")
P, L, CALLS = [200, 220, 250], 20, 10
SHAPES = {"cfg2": dict(tables=1, B=512, q=[4, 4, 4], ranks=[32, 32]),
          "cfg4": dict(tables=1, B=512, q=[4, 4, 8], ranks=[64, 64]),
          "cfg5 shard": dict(tables=4, B=4096, q=[4, 4, 4], ranks=[32, 32])}


def window(fn, steps):
    """device ms per call of fn over one window between two HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternate(fns, windows, steps):
    for fn in fns.values():
        window(fn, max(3, steps // 5))
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window(fn, steps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def captured(fn, calls):
    fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(calls):
            keep = fn()
    g._keep = keep
    return g


def bench(name, cfg, windows, steps):
    tables, B, q, ranks = cfg["tables"], cfg["B"], cfg["q"], cfg["ranks"]
    rr = [1] + ranks + [1]
    Erows, D = int(np.prod(P)), int(np.prod(q))
    nnz = tables * B * L
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, Erows, D, ranks, P, q, weight_dist="uniform", device=dev)
    inf = ttx_infer.TTInferenceBag.from_module(m)
    assert inf.route == "bf16"
    rs = np.random.RandomState(0)
    idx = torch.from_numpy(rs.randint(0, Erows, size=nnz).astype(np.int64)).to(dev)
    off = torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    _, tab, _ = E.lookup_prologue(idx, off, tables, P, q, rr)
    plan = E.make_plan(tables, P, q, rr, nnz, idx, tab, None)
    cores = [c.detach() for c in m.tt_cores]
    packed = inf._packed()
    f32 = lambda: E.tt_rows_p(tables, D, P, q, rr, idx, tab, cores, plan)  # noqa: E731
    b16 = lambda: E.tt_rows_bf16(tables, D, P, q, rr, idx, tab, packed, plan)  # noqa: E731
    r32, r16 = f32(), b16()
    qerr = float((r16 - r32).abs().max() / r32.abs().max())
    # bytes by the shapes: every distinct slice read once (an upper bound: all slices of the cores), the rows written
    slices = [tables * P[t] * rr[t] * q[t] * rr[t + 1] for t in range(3)]
    wr = nnz * D * 4
    print(f"[{name}] {nnz} lookups, D {D}, ranks {ranks}: rows written {wr / 1e6:.1f} MB; cores fp32 {4 * sum(slices) / 1e6:.1f} MB, "
          f"packed bf16 {2 * sum(x.numel() for x in packed) / 1e6:.1f} MB; quantisation error max|bf16 - fp32| / max|fp32| = {qerr:.3e}",
          flush=True)
    g32, g16 = captured(f32, CALLS), captured(b16, CALLS)
    res = alternate({"fp32 tt_rows_p": g32.replay, "bf16 tt_rows_bf16": g16.replay}, windows, steps)
    for k, (med, lo, hi) in res.items():
        nb = wr + (4 * sum(slices) if k.startswith("fp32") else 2 * sum(x.numel() for x in packed))
        print(f"[{name}] rows    {k:18s} median {med / CALLS * 1e3:8.2f} us/call (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f})  "
              f"{nb / (med / CALLS * 1e-3) / 1e12:6.3f} TB/s by the shapes", flush=True)

    def src():
        with torch.no_grad():
            return m(idx, off)

    fwd = {"source no_grad forward": src, "TTInferenceBag forward": lambda: inf(idx, off)}
    for k, (med, lo, hi) in alternate(fwd, windows, steps).items():
        print(f"[{name}] forward eager    {k:24s} median {med * 1e3:8.2f} us/call (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})", flush=True)
    gf = {k: captured(f, CALLS).replay for k, f in fwd.items()}
    for k, (med, lo, hi) in alternate(gf, windows, steps).items():
        print(f"[{name}] forward captured {k:24s} median {med / CALLS * 1e3:8.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
              f"max {hi / CALLS * 1e3:.2f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only", default=None, help="one of: " + ", ".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    print(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; windows {a.windows}, steps per window {a.steps}, "
          f"{CALLS} calls per captured graph")
    for name, cfg in SHAPES.items():
        if a.only in (None, name):
            bench(name, cfg, a.windows, a.steps)
