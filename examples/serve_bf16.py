#!/usr/bin/env python3
"""Compress a dense table, freeze it for serving in bf16, serve a batch:

    python examples/serve_bf16.py            # on cuda:0
    python examples/serve_bf16.py --wide     # TT ranks 96: the column-blocked bf16 kernel (route "bf16w")
    python examples/serve_bf16.py --mfma-tail  # D = 1024, q = [8, 8, 16]: both products on the bf16 MFMA (route "bf16m")
    python examples/serve_bf16.py --four-cores  # D = 256, q = [4, 4, 4, 4]: a four-core table on the bf16 MFMA (route "bf16q")
    python examples/serve_bf16.py --hot 4096   # keep the 4096 most visited rows of a skewed stream expanded
    python examples/serve_bf16.py --fused-bags  # one pooled launch per call, no plan and no rows (route "bf16b")

1. a dense table (low TT rank plus noise) stands in for a trained nn.EmbeddingBag;
2. `TTEmbeddingBag.from_pretrained` factors it by TT-SVD into an ordinary module;
3. `TTInferenceBag.from_module` freezes that module: the cores rounded once to bf16, no Parameters, forward only -- the lookups
   run on the bf16 MFMA with fp32 accumulation (`served.route == "bf16"`; a geometry the kernel does not take says "fp32" and
   serves the same rounded weights through the fp32 kernels; `from_module(trained, wide=True)` opts in to the column-blocked
   bf16 kernel for ranks up to 128 and wide q1: `served.route == "bf16w"`; `from_module(trained, mfma_tail=True)` to the
   kernel for a last factor q2 up to 32, the default factorings of widths from 640 up: `served.route == "bf16m"`;
   `from_module(trained, four_cores=True)` to the kernel for four-core tables: `served.route == "bf16q"`);
4. a batch is served and compared with the fp32 module and with the dense table;
5. with `--hot N` the stream is skewed (Zipf 1.2) and `from_module(trained, hot_indices=...)` keeps its N most visited rows as bf16
   rows beside the cores: their lookups are pooled from that table, only the misses are contracted."""
import argparse
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide", action="store_true", help="factor at TT ranks 96 and serve on the column-blocked bf16 kernel")
    ap.add_argument("--mfma-tail", action="store_true", help="a table of width 1024 (q = [8, 8, 16]) served on the MFMA-tail bf16 kernel")
    ap.add_argument("--four-cores", action="store_true", help="a four-core table of width 256 (q = [4, 4, 4, 4]) served on the four-core bf16 kernel")
    ap.add_argument("--hot", type=int, default=0, metavar="N", help="serve the N most visited rows of a Zipf 1.2 stream from a hot row table")
    ap.add_argument("--fused-bags", action="store_true", help="serve every call as ONE pooled launch (also takes per_sample_weights / padding_idx)")
    args = ap.parse_args()
    wide, tail, four = args.wide, args.mfma_tail, args.four_cores
    import tt_embeddings_ops as ops
    import ttx_infer
    import ttx_svd

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, D, p, q = (5_000, 1024, [10, 20, 25], [8, 8, 16]) if tail else (100_000, 64, [40, 50, 50], [4, 4, 4])
    if four:
        E, D, p, q = 50_000, 256, [10, 10, 20, 25], [4, 4, 4, 4]
    r = [1] + [8] * (len(p) - 1) + [1]
    cores = [torch.randn(r[k], p[k], q[k], r[k + 1], device=dev) / r[k] ** 0.5 for k in range(len(p))]
    weight = ttx_svd.tt_full(cores, E)
    weight += torch.randn_like(weight) * (0.02 * weight.norm() / weight.numel() ** 0.5)
    bag = nn.EmbeddingBag.from_pretrained(weight, freeze=True, mode="sum", include_last_offset=True)

    trained = ops.TTEmbeddingBag.from_pretrained(weight, [96, 96] if wide else [16] * (len(p) - 1), p, q, device=dev, use_cache=False)
    B, L = 512, 8
    idx = torch.randint(0, E, (B * L,), device=dev)
    hot = None
    if args.hot > 0:  # a skewed stream, and its most visited rows (in production: counted over yesterday's traffic)
        ranks = torch.from_numpy((np.random.RandomState(0).zipf(1.2, size=B * L) - 1) % E).to(dev)
        idx = torch.randperm(E, device=dev)[ranks]
        rows, counts = torch.unique(idx, return_counts=True)
        hot = rows[torch.argsort(counts, descending=True)[:args.hot]]
    served = ttx_infer.TTInferenceBag.from_module(trained, wide=wide, mfma_tail=tail, four_cores=four, hot_indices=hot,
                                                  fused_bags=args.fused_bags)
    print(served)
    if hot is not None:
        print(f"hot rows {served.hot_rows_count}: {torch.isin(idx, hot).float().mean().item():.1%} of the batch's lookups are served from them")
    print(f"route {served.route}; parameters {len(list(served.parameters()))}; "
          f"buffers {sum(b.numel() * b.element_size() for b in served.buffers()) / 1e3:.0f} kB "
          f"(fp32 cores: {sum(c.numel() * 4 for c in trained.tt_cores) / 1e3:.0f} kB, dense table: {weight.numel() * 4 / 1e6:.1f} MB)")

    off = torch.arange(0, B * L + 1, L, device=dev)
    out = served(idx, off)
    with torch.no_grad():
        fp32 = trained(idx, off)
    dense = bag(idx, off)
    scale = dense.abs().max()
    print(f"served {tuple(out.shape)} {out.dtype}, requires_grad={out.requires_grad}")
    print(f"max |bf16 - fp32 module| / max |row| = {((out - fp32).abs().max() / scale).item():.2e}   (the rounding of the cores)")
    print(f"max |bf16 - dense table| / max |row| = {((out - dense).abs().max() / scale).item():.2e}   (plus the TT truncation)")


if __name__ == "__main__":
    main()
