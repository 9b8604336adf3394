#!/usr/bin/env python3
"""Compress a trained nn.EmbeddingBag into a TT module, fine-tune it, lower its ranks:

    python examples/compress_pretrained.py            # on cuda:0

1. an nn.EmbeddingBag stands in for a trained table (low TT rank plus noise, so that there is something to find);
2. `TTEmbeddingBag.from_pretrained(bag.weight, rel_error=..)` factors it by TT-SVD -- the ranks are chosen for the error asked
   for -- and `from_pretrained(bag.weight, tt_ranks=[..])` at fixed ranks; `module.compression` reports ranks, bound and norm;
3. the module is an ordinary one: a few fused-SGD steps toward a target;
4. `truncate_ranks` rounds the trained cores to lower ranks and returns a new module."""
import os
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))


def main():
    import tt_embeddings_ops as ops
    import ttx_svd

    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    E, D, p, q = 100_000, 64, [40, 50, 50], [4, 4, 4]
    # a "trained" table: TT ranks [8, 8] plus 2 % noise
    r = [1, 8, 8, 1]
    cores = [torch.randn(r[k], p[k], q[k], r[k + 1], device=dev) / r[k] ** 0.5 for k in range(3)]
    weight = ttx_svd.tt_full(cores, E)
    weight += torch.randn_like(weight) * (0.02 * weight.norm() / weight.numel() ** 0.5)
    bag = nn.EmbeddingBag.from_pretrained(weight, freeze=False, mode="sum", include_last_offset=True)

    def report(what, m):
        ranks, bound, norm = m.compression[0]
        err = (m.full_weight(0) - bag.weight.detach()).norm().item()
        n_tt, n_dense = sum(c.numel() for c in m.tt_cores), bag.weight.numel()
        print(f"{what}: ranks {ranks}, ||W - TT|| / ||W|| = {err / norm:.4f} (the bound of its own factorisation: {bound / norm:.4f}), "
              f"{n_dense / n_tt:.0f}x fewer parameters")

    kw = dict(device=dev, use_cache=False, optimizer=ops.OptimType.SGD, learning_rate=0.005)
    chosen = ops.TTEmbeddingBag.from_pretrained(bag.weight, None, p, q, rel_error=0.05, max_rank=32, rank_multiple=8, **kw)
    report("rel_error=0.05", chosen)
    fixed = ops.TTEmbeddingBag.from_pretrained(bag.weight, [16, 16], p, q, **kw)
    report("tt_ranks=[16, 16]", fixed)

    # the compressed module against the bag it came from, then a few fused-SGD steps toward the bag's rows plus one
    B, L = 512, 8
    idx = torch.randint(0, E, (B * L,), device=dev)
    off = torch.arange(0, B * L + 1, L, device=dev)
    target = bag(idx, off).detach() + 1.0
    for step in range(5):
        out = fixed(idx, off)
        loss = 0.5 * (out - target).square().sum() / B
        print(f"step {step}: loss {loss.item():.4f}")
        out.backward((out.detach() - target) / B)  # (the fused optimizer applies the update inside backward)

    low = fixed.truncate_ranks([8, 8])
    report("truncate_ranks([8, 8]) of the fine-tuned module, against the original table", low)
    print("forward of the rounded module:", tuple(low(idx, off).shape))


if __name__ == "__main__":
    main()
