"""The column-blocked bf16 inference forward (TTInferenceBag.from_module(m, wide=True)) on an MI355X, by the
method of scripts/bench_bf16_forward.py (whose helpers it uses): HIP events around replays of a captured graph of CALLS calls,
the variants alternating in one process after a warm-up, medians of the windows with their min and max.

  rows     `tt_rows_bf16w` against `tt_rows_p` (the fp32 rows kernel route "fp32" runs for these shapes) on the SAME plan and
           the SAME rounded cores
  forward  the whole captured TTInferenceBag forward, wide=True against wide=False

Shapes: ranks 128 (q [4,4,4], cfg2's p) at 10,240 and 327,680 lookups; wide q1 (q [4,64,4], ranks [32,64]) at 10,240.

    python scripts/bench_bf16_wide.py [--windows 5] [--steps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bf16_forward import CALLS, E, L, P, alternate, captured, dev, ops, ttx_infer  # noqa: E402

SHAPES = {"r128 10k": dict(tables=1, B=512, q=[4, 4, 4], ranks=[128, 128]),
          "r128 327k": dict(tables=4, B=4096, q=[4, 4, 4], ranks=[128, 128]),
          "q1=64 10k": dict(tables=1, B=512, q=[4, 64, 4], ranks=[32, 64])}


def bench(name, cfg, windows, steps):
    tables, B, q, ranks = cfg["tables"], cfg["B"], cfg["q"], cfg["ranks"]
    rr = [1] + ranks + [1]
    Erows, D = int(np.prod(P)), int(np.prod(q))
    nnz = tables * B * L
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, Erows, D, ranks, P, q, weight_dist="uniform", device=dev)
    narrow, wide = ttx_infer.TTInferenceBag.from_module(m), ttx_infer.TTInferenceBag.from_module(m, wide=True)
    assert narrow.route == "fp32" and wide.route == "bf16w"
    rs = np.random.RandomState(0)
    idx = torch.from_numpy(rs.randint(0, Erows, size=nnz).astype(np.int64)).to(dev)
    off = torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    _, tab, _ = E.lookup_prologue(idx, off, tables, P, q, rr)
    plan = E.make_plan(tables, P, q, rr, nnz, idx, tab, None)
    cores = [c.detach() for c in narrow.fp32.tt_cores]  # (the rounded weights as fp32: what route "fp32" serves)
    packed = wide._packed()
    f32 = lambda: E.tt_rows_p(tables, D, P, q, rr, idx, tab, cores, plan)  # noqa: E731
    b16 = lambda: E.tt_rows_bf16w(tables, D, P, q, rr, idx, tab, packed, plan)  # noqa: E731
    r32, r16 = f32(), b16()
    diff = float((r16 - r32).abs().max() / r32.abs().max())
    macs = nnz * (q[0] * ranks[0] * q[1] * ranks[1] + q[0] * q[1] * ranks[1] * q[2])
    print(f"[{name}] {nnz} lookups, q {q}, ranks {ranks}: {2 * macs / 1e9:.1f} GFLOP per call; max|bf16w - fp32 kernel| / max|row| = "
          f"{diff:.3e} (same cores: summation order only)", flush=True)
    res = alternate({"fp32 tt_rows_p": captured(f32, CALLS).replay, "bf16w tt_rows_bf16w": captured(b16, CALLS).replay}, windows, steps)
    for k, (med, lo, hi) in res.items():
        print(f"[{name}] rows    {k:20s} median {med / CALLS * 1e3:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f})  "
              f"{2 * macs / (med / CALLS * 1e-3) / 1e12:6.2f} TFLOP/s", flush=True)
    gf = {"forward wide=False (fp32)": captured(lambda: narrow(idx, off), CALLS).replay,
          "forward wide=True (bf16w)": captured(lambda: wide(idx, off), CALLS).replay}
    for k, (med, lo, hi) in alternate(gf, windows, steps).items():
        print(f"[{name}] captured {k:26s} median {med / CALLS * 1e3:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
              f"max {hi / CALLS * 1e3:.2f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", default=None, help="one of: " + ", ".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    print(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; windows {a.windows}, steps per window {a.steps}, "
          f"{CALLS} calls per captured graph")
    for name, cfg in SHAPES.items():
        if a.only in (None, name):
            bench(name, cfg, a.windows, a.steps)
