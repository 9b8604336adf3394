#!/usr/bin/env python3
"""Does ONE row cache over tables of DIFFERENT cardinality pay?  The eight tables of four row shapes of scripts/bench_mixed.py
(10 M, 5 M, 1 M and 300 k rows, twice; q = [4, 4, 4], ranks 32, 512 bags of 20 lookups per table: 81,920 lookups per step, eager
forward + backward with fused SGD) on a Zipf(1.2) stream, three configurations ALTERNATED in one process, every one timed over
the same batches in DLRM's call form (one (indices, offsets) pair per table):

  var_cache     MixedTTEmbeddingBag(fused=True, use_cache=True), live: one launch set and one cache of `--cache-rows` rows
  no_cache      the same module with use_cache=False
  eight_caches  eight TTEmbeddingBag(use_cache=True), live, `--cache-rows` split in proportion to the cardinalities: one module
                and one launch set per table

A step is timed with device events around `--steps` steps after a warm-up of every configuration; `--rounds` rounds, the median
and the extremes of the per-round ms / step are reported.  The hit share is what the live preprocess leaves on the device for the
timed batches (1 - misses / lookups).
usage (GPU box): python scripts/bench_var_cache.py [--cache-rows 65536,1048576] [--bags 512] > var_cache.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import tt_embeddings as E  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_mixed  # noqa: E402

D, Q, RANKS, B, L = 64, [4, 4, 4], [32, 32], 512, 20  # (B: --bags)
SHAPES = {10_000_000: [200, 220, 250], 5_000_000: [160, 180, 200], 1_000_000: [100, 100, 100], 300_000: [64, 70, 72]}
ES = [10_000_000, 5_000_000, 1_000_000, 300_000] * 2
PS = [SHAPES[e] for e in ES]
NT = len(ES)
DEV = torch.device("cuda:0")


def batches(n, seed):
    """n batches: per table B bags of L lookups, indices Zipf(1.2) - 1 folded into the table (row 0 the hottest of every table)"""
    rs = np.random.RandomState(seed)
    off = [torch.arange(0, B * L, L, dtype=torch.int64, device=DEV) for _ in ES]
    out = []
    for _ in range(n):
        idx = [torch.from_numpy(((rs.zipf(1.2, size=B * L) - 1) % e).astype(np.int64)).to(DEV) for e in ES]
        out.append((idx, off))
    return out


def timed(step, todo, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for s in range(steps):
        step(*todo[s % len(todo)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    global B
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-rows", default="65536,1048576", help="total cache rows, one run per value")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-batches", type=int, default=12, help="batches counted before the populate")
    ap.add_argument("--bags", type=int, default=B, help="bags per table and step (20 lookups each)")
    a = ap.parse_args()
    B = a.bags
    kw = dict(optimizer=ops.OptimType.SGD, learning_rate=0.01, sparse=True, weight_dist="uniform", device=DEV)
    warm, todo = batches(a.warm_batches, 1), batches(8, 2)
    grads = [torch.rand(B, D, device=DEV) * 0.1 for _ in ES]
    closed = torch.arange(0, B * L + 1, L, dtype=torch.int64, device=DEV)
    out = []
    for rows in [int(x) for x in a.cache_rows.split(",")]:
        H = 4 * rows
        torch.manual_seed(0)
        vc = ttx_mixed.MixedTTEmbeddingBag(ES, D, RANKS, PS, Q, fused=True, use_cache=True, cache_size=rows, hashtbl_size=H, **kw)
        nc = ttx_mixed.MixedTTEmbeddingBag(ES, D, RANKS, PS, Q, fused=True, **kw)
        assert len(vc.groups) == 1 and len(nc.groups) == 1
        share = [max(1, rows * e // sum(ES)) for e in ES]
        eight = [ops.TTEmbeddingBag(ES[k], D, RANKS, PS[k], Q, use_cache=True, cache_size=share[k], hashtbl_size=4 * share[k],
                                    include_last_offset=False, **kw) for k in range(NT)]
        with torch.no_grad():
            for idx, off in warm:
                vc(idx, off)
                for m, i, o in zip(eight, idx, off):
                    m(i, o)
        vc.cache_populate()
        for m in eight:
            m.cache_populate()

        def step_vc(idx, off):
            torch.autograd.backward(vc(idx, off), grads)

        def step_nc(idx, off):
            torch.autograd.backward(nc(idx, off), grads)

        def step_eight(idx, off):
            torch.autograd.backward([m(i, o) for m, i, o in zip(eight, idx, off)], grads)

        configs = {"var_cache": step_vc, "no_cache": step_nc, "eight_caches": step_eight}
        for step in configs.values():  # warm-up of every configuration (allocator, lazy initialisation)
            timed(step, todo, 4)
        ms = {k: [] for k in configs}
        for _ in range(a.rounds):  # alternated: one round times every configuration once
            for k, step in configs.items():
                ms[k].append(timed(step, todo, a.steps))
        # hit shares of the timed batches (the live preprocess's split point, read back outside the timing; nothing is counted)
        g = vc.groups[0]
        miss_vc = miss_eight = 0
        for idx, off in todo:
            mi, mo = ttx_mixed.merge_bags(idx, off, False)
            keys = E.table_keys(mi, mo, NT, g._key_space())
            miss_vc += int(E.preprocess_indices_async(keys, mo, g.hashtbl, g.cache_state)[3].item())
            for m, i in zip(eight, idx):
                miss_eight += int(E.preprocess_indices_async(i, closed, m.hashtbl, m.cache_state)[3].item())
        n = len(todo) * NT * B * L
        rec = {"cache_rows_total": rows, "hashtbl_slots_total": H, "lookups_per_step": NT * B * L, "steps": a.steps, "rounds": a.rounds,
               "hit_share": {"var_cache": round(1 - miss_vc / n, 4), "eight_caches": round(1 - miss_eight / n, 4)},
               "cached_keys": {"var_cache": int((g.cache_state >= 0).sum()), "eight_caches": sum(int((m.cache_state >= 0).sum()) for m in eight)}}
        for k, v in ms.items():
            rec[k] = {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4),
                      "rounds_ms": [round(x, 4) for x in v]}
        out.append(rec)
        del vc, nc, eight
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
