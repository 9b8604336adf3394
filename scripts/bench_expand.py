"""The expand kernel (`dense_rows`) on an MI355X, by the method of scripts/bench_bf16_forward.py (whose helpers
it uses): HIP events around replays of a captured graph of CALLS calls, the variants alternating in one process after a warm-up,
medians of the windows with their min and max.

  expand   `tt_expand` into a resident output: one launch, no indices
  rows     what served a range before it: `tt_rows` over a resident arange of the same range, its plan build included
  tt_full  (whole cfg2 table only, eager, events around each call) the torch-op expansion behind `full_weight`

Shapes: cfg2's table (q [4,4,4], ranks 32) 2^20 rows from row 0 and from an unaligned start, 1,024 rows (the few-prefix split),
cfg4's table (q [4,4,8], ranks 64) 2^20 rows.  Reported per call: time, the row store's bytes/s against 8 TB/s and product 2's
FLOP/s (2 q0 q1 r2 q2 per row) against 157 TFLOP/s (DESIGN.md section 4's figures).

    python scripts/bench_expand.py [--windows 5] [--steps 10] [--no-full]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bf16_forward import E, P, alternate, captured, dev, ops  # noqa: E402
import ttx_svd  # noqa: E402

CALLS = 4
SHAPES = {"cfg2 2^20 from 0": dict(q=[4, 4, 4], ranks=[32, 32], start=0, n=1 << 20),
          "cfg2 2^20 unaligned": dict(q=[4, 4, 4], ranks=[32, 32], start=1234567, n=1 << 20),
          "cfg2 1024 rows": dict(q=[4, 4, 4], ranks=[32, 32], start=1234567, n=1024),
          "cfg4 2^20 from 0": dict(q=[4, 4, 8], ranks=[64, 64], start=0, n=1 << 20)}


def bench(name, cfg, windows, steps):
    q, ranks, start, n = cfg["q"], cfg["ranks"], cfg["start"], cfg["n"]
    rr, D = [1] + ranks + [1], int(np.prod(q))
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(1, int(np.prod(P)), D, ranks, P, q, weight_dist="uniform", device=dev)
    cores = [c.detach() for c in m.tt_cores]
    idx = torch.arange(start, start + n, dtype=torch.int64, device=dev)
    out = torch.empty((n, D), dtype=torch.float32, device=dev)
    new = lambda: E.tt_expand(1, D, P, q, rr, 0, start, start + n, cores, out)  # noqa: E731
    old = lambda: E.tt_rows(1, D, P, q, rr, idx, None, cores)  # noqa: E731
    a, b = new().clone(), old()
    print(f"[{name}] {n} rows of {D}: max|expand - rows kernel| / max|row| = {float((a - b).abs().max() / b.abs().max()):.3e} "
          f"(same cores: summation order only)", flush=True)
    res = alternate({"expand tt_expand": captured(new, CALLS).replay, "rows tt_rows(arange)": captured(old, CALLS).replay}, windows, steps)
    flop = 2.0 * n * D * ranks[1]
    for k, (med, lo, hi) in res.items():
        s = med / CALLS * 1e-3
        print(f"[{name}] {k:22s} median {s * 1e6:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f})  store "
              f"{4.0 * n * D / s / 1e12:5.2f} TB/s ({4.0 * n * D / s / 8e12:5.1%} of 8 TB/s)  product 2 {flop / s / 1e12:6.2f} TFLOP/s "
              f"({flop / s / 157e12:5.1%} of 157)", flush=True)
    (en, eo), (sn, so) = ((res[k][0], res[k][2] - res[k][1]) for k in res)
    print(f"[{name}] rows / expand = {sn / en:.2f}x; difference {(sn - en) / CALLS * 1e3:.2f} us against the two spreads' sum "
          f"{(eo + so) / CALLS * 1e3:.2f} us", flush=True)
    return m


def bench_full(m, reps):
    """the whole cfg2 table: dense_rows (one launch) against ttx_svd.tt_full (torch ops: two copies of the table), eager"""
    def timed(fn):
        ts = []
        for _ in range(reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            keep = fn()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
            del keep
        return statistics.median(ts[1:]), min(ts[1:]), max(ts[1:])

    out = torch.empty((m.num_embeddings, m.embedding_dim), dtype=torch.float32, device=dev)
    for k, fn in (("dense_rows (whole table)", lambda: m.dense_rows(out=out)), ("tt_full (whole table)", lambda: ttx_svd.tt_full(m.table_cores(0)))):
        med, lo, hi = timed(fn)
        print(f"[cfg2 whole table] {k:26s} median {med:9.2f} ms (min {lo:.2f}, max {hi:.2f})  {out.numel() * 4 / med / 1e9:5.2f} TB/s stored",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-full", action="store_true", help="skip the whole-table comparison with tt_full")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    print(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; windows {a.windows}, steps per window {a.steps}, "
          f"{CALLS} calls per captured graph")
    mods = {name: bench(name, cfg, a.windows, a.steps) for name, cfg in SHAPES.items()}
    if not a.no_full:
        bench_full(mods["cfg2 2^20 from 0"], 3)
