"""The four-core bf16 inference forward (TTInferenceBag.from_module(m, four_cores=True)) on an MI355X, by the
method of scripts/bench_bf16_mfma.py: HIP events around replays of a captured graph of CALLS calls, the variants alternating in
one process after a warm-up, medians of the windows with their min and max.

  rows     `tt_rows_bf16q` against `tt_rows_p` (the fp32 four-core rows route: the merged last cores through the plan, then a
           three-core kernel) on the SAME plan and the SAME rounded cores; the row-store floor (bytes of rows over 8 TB/s) and the
           fraction of it reached; the worst err / bound of the first 256 lookups against float64 (tests/bf16q_ref.py)
  forward  the whole captured TTInferenceBag forward, four_cores=True against four_cores=False (route "fp32")

Shapes: bench.py's t4 (q [2,4,4,2]) and t4d256 (q [4,4,4,4]), ranks 32, p [58,58,58,58], at 10,240 and 327,680 lookups.

    python scripts/bench_bf16_quad.py [--windows 5] [--steps 20]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_bf16_forward import CALLS, ROOT, E, alternate, captured, dev, ops, ttx_infer  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
import bf16q_ref as Q  # noqa: E402

HBM = 8e12  # bytes / s
L = 20      # lookups per bag
P = [58, 58, 58, 58]
RANKS = [32, 32, 32]
SHAPES = {"t4 10k": dict(B=512, q=[2, 4, 4, 2]), "t4 328k": dict(B=16384, q=[2, 4, 4, 2]),
          "t4d256 10k": dict(B=512, q=[4, 4, 4, 4]), "t4d256 328k": dict(B=16384, q=[4, 4, 4, 4])}


def bench(name, cfg, windows, steps):
    B, q, tables = cfg["B"], cfg["q"], 1
    rr = [1] + RANKS + [1]
    Erows, D = int(np.prod(P)), int(np.prod(q))
    nnz = tables * B * L
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, Erows, D, RANKS, P, q, weight_dist="uniform", device=dev)
    plain, quad = ttx_infer.TTInferenceBag.from_module(m), ttx_infer.TTInferenceBag.from_module(m, four_cores=True)
    assert plain.route == "fp32" and quad.route == "bf16q"
    rs = np.random.RandomState(0)
    idx = torch.from_numpy(rs.randint(0, Erows, size=nnz).astype(np.int64)).to(dev)
    off = torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    _, tab, _ = E.lookup_prologue(idx, off, tables, P, q, rr)
    plan = E.make_plan(tables, P, q, rr, nnz, idx, tab, None)
    cores = [c.detach() for c in plain.fp32.tt_cores]  # (the rounded weights as fp32: what route "fp32" serves)
    packed = quad._packed()
    f32 = lambda: E.tt_rows_p(tables, D, P, q, rr, idx, tab, cores, plan)  # noqa: E731
    b16 = lambda: E.tt_rows_bf16q(tables, D, P, q, rr, idx, tab, packed, plan)  # noqa: E731
    n = 256
    ref, bnd = Q.rows64(*Q.slices([c.cpu().numpy() for c in cores], P, q, RANKS, idx[:n].cpu().numpy(), tab[:n].cpu().numpy()))
    ratio = [float(np.max(np.abs(f()[:n].cpu().numpy().astype(np.float64) - ref) / np.maximum(bnd, 1e-300))) for f in (f32, b16)]
    r1, r2, r3 = RANKS
    macs = nnz * (q[0] * r1 * q[1] * r2 + r2 * q[2] * r3 * q[3] + q[0] * q[1] * r2 * q[2] * q[3])  # chain order
    floor = nnz * D * 4 / HBM * 1e6
    print(f"[{name}] {nnz} lookups, q {q}, ranks {RANKS}: {2 * macs / 1e9:.2f} GFLOP per call in chain order; row-store floor "
          f"{floor:.2f} us; worst err / bound over {n} lookups: fp32 route {ratio[0]:.5f}, bf16q {ratio[1]:.5f}", flush=True)
    res = alternate({"fp32 tt_rows_p": captured(f32, CALLS).replay, "bf16q tt_rows_bf16q": captured(b16, CALLS).replay}, windows, steps)
    for k, (med, lo, hi) in res.items():
        us = med / CALLS * 1e3
        print(f"[{name}] rows    {k:20s} median {us:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f})  "
              f"floor / time {floor / us:.3f}", flush=True)
    gf = {"forward four_cores=False (fp32)": captured(lambda: plain(idx, off), CALLS).replay,
          "forward four_cores=True (bf16q)": captured(lambda: quad(idx, off), CALLS).replay}
    for k, (med, lo, hi) in alternate(gf, windows, steps).items():
        print(f"[{name}] captured {k:32s} median {med / CALLS * 1e3:9.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
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
