#!/usr/bin/env python3
"""The cache refresh at cfg3's size (hashtbl_size 2^20, 262,144 cache rows, D = 64): the time of
cache_populate(keep_trained=True) beside cache_populate() -- alternated, a counted batch between two populates so that keys
enter and leave -- and ttx_cache_carry alone with the bytes it moves against the 8 TB/s HBM3E peak.  HIP events, warm-up first,
medians of --runs runs.  On a build without the feature only the plain populate is timed.
usage (on the GPU): python scripts/bench_cache_refresh.py [--runs 21] > cache_refresh.json"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
import inspect

import numpy as np
import torch
import tt_embeddings as E
import tt_embeddings_ops as ops

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=21)
args = ap.parse_args()
dev = torch.device("cuda:0")
E_, D, H, CS, PEAK = 11_000_000, 64, 1 << 20, 1 << 18, 8000.0
torch.manual_seed(1)
m = ops.TTEmbeddingBag(E_, D, [32, 32], [200, 220, 250], [4, 4, 4], sparse=True, optimizer=ops.OptimType.EXACT_ROWWISE_ADAGRAD,
                       learning_rate=0.05, use_cache=True, cache_size=CS, hashtbl_size=H, weight_dist="uniform", device=dev)
has_feature = "keep_trained" in inspect.signature(m.cache_populate).parameters
rs = np.random.RandomState(2)


def count(n):  # a Zipf(1.2) batch into the frequency table
    m.update_cache(torch.from_numpy((rs.zipf(1.2, size=n).astype(np.int64) - 1) % E_).to(dev))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


for _ in range(8):
    count(1 << 20)
m.cache_populate()
variants = {"populate": lambda: m.cache_populate()}
if has_feature:
    variants["populate_keep_trained"] = lambda: m.cache_populate(keep_trained=True)
times = {k: [] for k in variants}
for run in range(-3, args.runs):  # (three warm-up rounds)
    for name, fn in variants.items():
        count(1 << 18)
        t = timed(fn)
        if run >= 0:
            times[name].append(t)
out = {"H": H, "cache_size": CS, "D": D, "runs": args.runs, "cached_keys": int((m.cache_state >= 0).sum()),
       "seated_keys": int((m.hashtbl >= 0).sum())}
for name, ts in times.items():
    out[name] = {"median_ms": round(statistics.median(ts) * 1e3, 4), "min_ms": round(min(ts) * 1e3, 4), "max_ms": round(max(ts) * 1e3, 4)}
if has_feature:
    # the carry alone, on the states of a real refresh: row-wise state, as the module hands it over
    count(1 << 18)
    old_state, old_w = m.cache_state.clone(), m.cache_weight.detach().clone()
    old_s = m._cache_row_state().clone()
    m.cache_populate()
    new_state, w, s = m.cache_state, m.cache_weight.detach(), m._cache_row_state()
    part = (m.hashtbl != -1) & (new_state >= 0)
    kept = int((part & (old_state >= 0)).sum())  # (upper bound: second copies of a key take no part)
    ts = []
    for run in range(-3, args.runs):
        t = timed(lambda: E.cache_carry(m.hashtbl, old_state, new_state, old_w, w, old_s, s))
        if run >= 0:
            ts.append(t)
    med = statistics.median(ts)
    nbytes = 16 * H + 8 * D * kept + 8 * int(part.sum())
    out["carry"] = {"median_us": round(med * 1e6, 2), "min_us": round(min(ts) * 1e6, 2), "max_us": round(max(ts) * 1e6, 2),
                    "participants": int(part.sum()), "kept": kept, "bytes": nbytes, "GB/s": round(nbytes / med / 1e9, 1),
                    "frac_of_8TB/s": round(nbytes / med / 1e9 / PEAK, 4)}
    clones = timed(lambda: (m.cache_state.clone(), m.cache_weight.detach().clone(), m._cache_row_state().clone()))
    out["clones_us"] = round(clones * 1e6, 2)
print(json.dumps(out, indent=1))
