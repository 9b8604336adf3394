#!/usr/bin/env python3
"""Does ONE row cache over the tables of a table-batched bag pay?  Four tables of cfg5's per-GPU shard shape (p = [200, 220, 250],
q = [4, 4, 4], ranks 32, 4096 bags of 20 lookups per table: 327,680 lookups per step, fused SGD) on a Zipf(1.2) stream, three
configurations ALTERNATED in one process, every one timed over the same batches:

  table_cache   TableBatchedTTEmbeddingBag(4 tables, use_cache=True), live: one cache of `--cache-rows` rows over all tables
  no_cache      the same module with use_cache=False
  four_caches   four TTEmbeddingBag(use_cache=True), live, `--cache-rows` / 4 rows each: one module and one launch set per table

A step is forward + backward (the fused optimizer inside), timed with device events around `--steps` steps after a warm-up of
every configuration; `--rounds` rounds, the median and the extremes of the per-round ms / step are reported.  The hit share is
what the live preprocess leaves on the device for the timed batches (1 - misses / lookups).
usage (GPU box): python scripts/bench_table_cache.py [--cache-rows 65536,1048576] > table_cache.json"""
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

P, Q, RANKS = [200, 220, 250], [4, 4, 4], [32, 32]
NT, B, L, D = 4, 4096, 20, 64
ROWS = int(np.prod(P))
DEV = torch.device("cuda:0")


def batches(n, seed):
    """n batches: per table B bags of L lookups, indices Zipf(1.2) - 1 folded into the table (row 0 the hottest of every table)"""
    rs = np.random.RandomState(seed)
    off = torch.arange(0, NT * B * L + 1, L, dtype=torch.int64, device=DEV)
    out = []
    for _ in range(n):
        idx = ((rs.zipf(1.2, size=NT * B * L) - 1) % ROWS).astype(np.int64)
        out.append((torch.from_numpy(idx).to(DEV), off))
    return out


def per_table(batch):
    idx, _ = batch
    off = torch.arange(0, B * L + 1, L, dtype=torch.int64, device=DEV)
    return [(idx[k * B * L:(k + 1) * B * L].contiguous(), off) for k in range(NT)]


def timed(step, todo, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for s in range(steps):
        step(todo[s % len(todo)])
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache-rows", default="65536,1048576", help="total cache rows, one run per value")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warm-batches", type=int, default=12, help="batches counted before the populate")
    a = ap.parse_args()
    kw = dict(optimizer=ops.OptimType.SGD, learning_rate=0.01, sparse=True, weight_dist="uniform", device=DEV)
    warm, todo = batches(a.warm_batches, 1), batches(8, 2)
    grad = torch.rand(NT, B, D, device=DEV) * 0.1
    grads = [grad[k].contiguous() for k in range(NT)]
    todo_t = [per_table(bt) for bt in todo]
    out = []
    for rows in [int(x) for x in a.cache_rows.split(",")]:
        H = 4 * rows
        torch.manual_seed(0)
        tc = ops.TableBatchedTTEmbeddingBag(NT, ROWS, D, RANKS, P, Q, use_cache=True, cache_size=rows, hashtbl_size=H, **kw)
        nc = ops.TableBatchedTTEmbeddingBag(NT, ROWS, D, RANKS, P, Q, use_cache=False, **kw)
        four = [ops.TTEmbeddingBag(ROWS, D, RANKS, P, Q, use_cache=True, cache_size=rows // NT, hashtbl_size=H // NT, **kw)
                for _ in range(NT)]
        with torch.no_grad():
            for bt in warm:
                tc(*bt)
                for m, (i, o) in zip(four, per_table(bt)):
                    m(i, o)
        tc.cache_populate()
        for m in four:
            m.cache_populate()

        def step_tc(bt):
            tc(*bt).backward(grad)

        def step_nc(bt):
            nc(*bt).backward(grad)

        def step_four(k):
            for m, (i, o), g in zip(four, todo_t[k], grads):
                m(i, o).backward(g)

        configs = {"table_cache": (step_tc, todo), "no_cache": (step_nc, todo), "four_caches": (step_four, list(range(len(todo))))}
        for step, td in configs.values():  # warm-up of every configuration (allocator, lazy initialisation)
            timed(step, td, 4)
        ms = {k: [] for k in configs}
        for _ in range(a.rounds):  # alternated: one round times every configuration once
            for k, (step, td) in configs.items():
                ms[k].append(timed(step, td, a.steps))
        # hit shares of the timed batches (the live preprocess's split point, read back outside the timing; nothing is counted)
        stride = tc._key_stride()
        miss_tc = miss_four = 0
        for bt, btt in zip(todo, todo_t):
            keys = E.table_keys(bt[0], bt[1], NT, stride)
            miss_tc += int(E.preprocess_indices_async(keys, bt[1], tc.hashtbl, tc.cache_state)[3].item())
            for m, (i, o) in zip(four, btt):
                miss_four += int(E.preprocess_indices_async(i, o, m.hashtbl, m.cache_state)[3].item())
        n = len(todo) * NT * B * L
        rec = {"cache_rows_total": rows, "hashtbl_slots_total": H, "lookups_per_step": NT * B * L, "steps": a.steps, "rounds": a.rounds,
               "hit_share": {"table_cache": round(1 - miss_tc / n, 4), "four_caches": round(1 - miss_four / n, 4)},
               "cached_keys": {"table_cache": int((tc.cache_state >= 0).sum()), "four_caches": sum(int((m.cache_state >= 0).sum()) for m in four)}}
        for k, v in ms.items():
            rec[k] = {"ms_per_step_median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        out.append(rec)
        del tc, nc, four
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
