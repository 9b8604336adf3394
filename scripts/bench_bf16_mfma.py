"""The MFMA-tail bf16 inference forward (TTInferenceBag.from_module(m, mfma_tail=True)) on an MI355X, by the
method of scripts/bench_bf16_wide.py (whose helpers it uses): HIP events around replays of a captured graph of CALLS calls, the
variants alternating in one process after a warm-up, medians of the windows with their min and max.

  rows     `tt_rows_bf16m` against `tt_rows_p` (the fp32 rows kernel route "fp32" runs for these shapes) on the SAME plan and
           the SAME rounded cores; the row-store floor (bytes of rows over 8 TB/s) and the fraction of it reached; the worst
           err / bound of the first 256 lookups against float64 (tests/bf16_ref.py)
  forward  the whole captured TTInferenceBag forward, mfma_tail=True against mfma_tail=False

Shapes: q [8,8,16] (D = 1024) at ranks 32 and 64, at 10,240 and 131,072 lookups; q [16,16,16] (D = 4096) at ranks 64, 32,768.

    python scripts/bench_bf16_mfma.py [--windows 5] [--steps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bf16_forward import CALLS, ROOT, E, P, alternate, captured, dev, ops, ttx_infer  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16_ref as R  # noqa: E402

HBM = 8e12  # bytes / s
L = 16      # lookups per bag
SHAPES = {"D1024 r32 10k": dict(tables=1, B=640, q=[8, 8, 16], ranks=[32, 32]),
          "D1024 r32 131k": dict(tables=1, B=8192, q=[8, 8, 16], ranks=[32, 32]),
          "D1024 r64 10k": dict(tables=1, B=640, q=[8, 8, 16], ranks=[64, 64]),
          "D1024 r64 131k": dict(tables=1, B=8192, q=[8, 8, 16], ranks=[64, 64]),
          "D4096 r64 32k": dict(tables=1, B=2048, q=[16, 16, 16], ranks=[64, 64])}


def bench(name, cfg, windows, steps):
    tables, B, q, ranks = cfg["tables"], cfg["B"], cfg["q"], cfg["ranks"]
    rr = [1] + ranks + [1]
    Erows, D = int(np.prod(P)), int(np.prod(q))
    nnz = tables * B * L
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, Erows, D, ranks, P, q, weight_dist="uniform", device=dev)
    plain, tail = ttx_infer.TTInferenceBag.from_module(m), ttx_infer.TTInferenceBag.from_module(m, mfma_tail=True)
    assert plain.route == "fp32" and tail.route == "bf16m"
    rs = np.random.RandomState(0)
    idx = torch.from_numpy(rs.randint(0, Erows, size=nnz).astype(np.int64)).to(dev)
    off = torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    _, tab, _ = E.lookup_prologue(idx, off, tables, P, q, rr)
    plan = E.make_plan(tables, P, q, rr, nnz, idx, tab, None)
    cores = [c.detach() for c in plain.fp32.tt_cores]  # (the rounded weights as fp32: what route "fp32" serves)
    packed = tail._packed()
    f32 = lambda: E.tt_rows_p(tables, D, P, q, rr, idx, tab, cores, plan)  # noqa: E731
    b16 = lambda: E.tt_rows_bf16m(tables, D, P, q, rr, idx, tab, packed, plan)  # noqa: E731
    n = 256
    ref, bnd = R.rows64(*R.slices([c.cpu().numpy() for c in cores], P, q, ranks, idx[:n].cpu().numpy(), tab[:n].cpu().numpy()))
    ratio = [float(np.max(np.abs(f()[:n].cpu().numpy().astype(np.float64) - ref) / np.maximum(bnd, 1e-300))) for f in (f32, b16)]
    macs = nnz * (q[0] * ranks[0] * q[1] * ranks[1] + q[0] * q[1] * ranks[1] * q[2])
    floor = nnz * D * 4 / HBM * 1e6
    print(f"[{name}] {nnz} lookups, q {q}, ranks {ranks}: {2 * macs / 1e9:.1f} GFLOP per call; row-store floor {floor:.2f} us; worst "
          f"err / bound over {n} lookups: fp32 kernel {ratio[0]:.5f}, bf16m {ratio[1]:.5f}", flush=True)
    res = alternate({"fp32 tt_rows_p": captured(f32, CALLS).replay, "bf16m tt_rows_bf16m": captured(b16, CALLS).replay}, windows, steps)
    for k, (med, lo, hi) in res.items():
        us = med / CALLS * 1e3
        print(f"[{name}] rows    {k:20s} median {us:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f})  "
              f"{2 * macs / (us * 1e-6) / 1e12:6.2f} TFLOP/s  floor / time {floor / us:.3f}", flush=True)
    gf = {"forward mfma_tail=False (fp32)": captured(lambda: plain(idx, off), CALLS).replay,
          "forward mfma_tail=True (bf16m)": captured(lambda: tail(idx, off), CALLS).replay}
    for k, (med, lo, hi) in alternate(gf, windows, steps).items():
        print(f"[{name}] captured {k:31s} median {med / CALLS * 1e3:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
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
