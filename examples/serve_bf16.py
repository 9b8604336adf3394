#!/usr/bin/env python3
"""Compress a dense table, freeze it for serving in bf16, serve a batch:

    python examples/serve_bf16.py            # on cuda:0

1. a dense table (low TT rank plus noise) stands in for a trained nn.EmbeddingBag;
2. `TTEmbeddingBag.from_pretrained` factors it by TT-SVD into an ordinary module;
3. `TTInferenceBag.from_module` freezes that module: the cores rounded once to bf16, no Parameters, forward only -- the lookups
   run on the bf16 MFMA with fp32 accumulation (`served.route == "bf16"`; a geometry the kernel does not take says "fp32" and
   serves the same rounded weights through the fp32 kernels);
4. a batch is served and compared with the fp32 module and with the dense table."""
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))


def main():
    import tt_embeddings_ops as ops
    import ttx_infer
    import ttx_svd

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, D, p, q = 100_000, 64, [40, 50, 50], [4, 4, 4]
    r = [1, 8, 8, 1]
    cores = [torch.randn(r[k], p[k], q[k], r[k + 1], device=dev) / r[k] ** 0.5 for k in range(3)]
    weight = ttx_svd.tt_full(cores, E)
    weight += torch.randn_like(weight) * (0.02 * weight.norm() / weight.numel() ** 0.5)
    bag = nn.EmbeddingBag.from_pretrained(weight, freeze=True, mode="sum", include_last_offset=True)

    trained = ops.TTEmbeddingBag.from_pretrained(weight, [16, 16], p, q, device=dev, use_cache=False)
    served = ttx_infer.TTInferenceBag.from_module(trained)
    print(served)
    print(f"route {served.route}; parameters {len(list(served.parameters()))}; "
          f"buffers {sum(b.numel() * b.element_size() for b in served.buffers()) / 1e3:.0f} kB "
          f"(fp32 cores: {sum(c.numel() * 4 for c in trained.tt_cores) / 1e3:.0f} kB, dense table: {weight.numel() * 4 / 1e6:.1f} MB)")

    B, L = 512, 8
    idx = torch.randint(0, E, (B * L,), device=dev)
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
