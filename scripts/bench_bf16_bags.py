"""The pooled one-launch bf16 forward (TTInferenceBag.from_module(m, fused_bags=True)) on an MI355X, against the same
module WITHOUT the flag (the plan-based route: prologue, rows kernel, pooling).

  captured  the TTInferenceBag forward as a captured graph of CALLS calls replayed: device microseconds per call between two HIP
            events
  eager     the same forward called from Python
  error     worst |fused - float64| / bound of tests/bf16b_ref.py on a sample of the batch's bags

Shapes: cfg2 (one table, q [4,4,4], ranks 32) and cfg4 (q [4,4,8], ranks 64) at 10,240 lookups, cfg5's per-GPU shard (4 tables,
327,680 lookups) in bags of 20, and cfg2 at a small serving batch of 512 lookups in bags of 16.  The variants alternate in one process after a
warm-up; medians of the windows with their min and max.  L2 bytes by the shapes: one core-1 slice per lookup.

    python scripts/bench_bf16_bags.py [--windows 7] [--steps 50] [--only cfg2]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tt_embeddings_ops as ops  # noqa: E402
import ttx_infer  # noqa: E402
from bench_bf16_forward import CALLS, P, alternate, captured, dev  # noqa: E402

SHAPES = {"cfg2": dict(tables=1, B=512, q=[4, 4, 4], ranks=[32, 32]),
          "cfg4": dict(tables=1, B=512, q=[4, 4, 8], ranks=[64, 64]),
          "cfg5 shard": dict(tables=4, B=4096, q=[4, 4, 4], ranks=[32, 32]),
          "cfg2 small": dict(tables=1, B=32, L=16, q=[4, 4, 4], ranks=[32, 32])}


def bench(name, cfg, windows, steps):
    import bf16_ref as R
    import bf16b_ref as RB

    tables, B, q, ranks, L = cfg["tables"], cfg["B"], cfg["q"], cfg["ranks"], cfg.get("L", 20)
    Erows, D = int(np.prod(P)), int(np.prod(q))
    nnz = tables * B * L
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, Erows, D, ranks, P, q, weight_dist="uniform", device=dev)
    plan, fused = ttx_infer.TTInferenceBag.from_module(m), ttx_infer.TTInferenceBag.from_module(m, fused_bags=True)
    assert plan.route == "bf16" and fused.route == "bf16b"
    rs = np.random.RandomState(0)
    idx_h = rs.randint(0, Erows, size=nnz).astype(np.int64)
    idx = torch.from_numpy(idx_h).to(dev)
    off = torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    # error of the first bags of every table against float64 on the same bf16 cores
    n = min(B, 16)
    out = fused(idx, off).cpu().numpy().astype(np.float64)
    cores = [R.to_bf16(c.detach().cpu().numpy()) for c in m.tt_cores]
    worst = 0.0
    for k in range(tables):
        sub = idx_h[k * B * L:(k * B + n) * L]
        one = [c[k:k + 1] for c in cores]
        ref, bnd = RB.bags64(one, P, q, ranks, 1, sub, np.arange(0, n * L + 1, L))
        worst = max(worst, float(np.max(np.abs(out[k, :n] - ref) / np.maximum(bnd, 1e-300))))
    K1p, K2p = -(-ranks[0] // 32) * 32, -(-ranks[1] // 32) * 32
    per = 2 * (q[0] * K1p + -(-q[1] * ranks[1] // 16) * 16 * K1p + -(-q[2] // 16) * 16 * K2p)
    print(f"[{name}] {nnz} lookups in {tables * B} bags, D {D}, ranks {ranks}: worst err / bound {worst:.4f}; fused route reads "
          f"{per} B of slices per lookup, {per * nnz / 1e6:.1f} MB per call by the shapes; output {tables * B * D * 4 / 1e6:.2f} MB", flush=True)
    fwd = {"plan-based (no flag)": lambda: plan(idx, off), "fused_bags=True": lambda: fused(idx, off)}
    for k, (med, lo, hi) in alternate(fwd, windows, steps).items():
        print(f"[{name}] forward eager    {k:22s} median {med * 1e3:8.2f} us/call (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})", flush=True)
    gf = {k: captured(f, CALLS).replay for k, f in fwd.items()}
    for k, (med, lo, hi) in alternate(gf, windows, steps).items():
        print(f"[{name}] forward captured {k:22s} median {med / CALLS * 1e3:8.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
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
