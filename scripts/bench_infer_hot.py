"""TTInferenceBag's hot row table on an MI355X: what serving the K hottest rows of a stream from an expanded bf16
table costs and saves.

  forward  the whole captured forward of a TTInferenceBag WITH the table against the same module WITHOUT one (the behaviour before
           the table existed): a captured graph of CALLS calls replayed, device microseconds per call between two HIP events
  launches every launch of the served call on its own, each a captured graph of CALLS launches on the inputs the one before it
           left: probe + pool, compaction, prologue on the live count, rows kernel, pool-add
  bytes    what the probe + pool launch moves by its shapes (indices read, masked indices written, 8 bytes each; the hit rows, 2 D
           bytes each; the hit sums written, 4 D bytes a bag) against its time

Shapes: cfg5's per-GPU shard (4 tables, 327,680 lookups) and cfg2 (one table, 10,240 lookups); traffic Zipf 1.2 (ranks scattered
over the table by a fixed permutation) and uniform; K = 65,536 hottest keys of the stream itself.  The variants alternate in one
process after a warm-up; medians of the windows with their min and max.

    python scripts/bench_infer_hot.py [--windows 5] [--steps 50] [--only "cfg2"]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import tt_embeddings as E  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_infer  # noqa: E402
from bench_bf16_forward import CALLS, L, P, alternate, captured  # noqa: E402

dev = torch.device("cuda:0")
K_HOT = 65536
SHAPES = {"cfg5 shard": dict(tables=4, B=4096, q=[4, 4, 4], ranks=[32, 32]), "cfg2": dict(tables=1, B=512, q=[4, 4, 4], ranks=[32, 32])}


def stream(rs, traffic, n, rows):
    if traffic == "uniform":
        return rs.randint(0, rows, size=n).astype(np.int64)
    return rs.permutation(rows)[(rs.zipf(1.2, size=n) - 1) % rows].astype(np.int64)


def bench(name, cfg, traffic, windows, steps):
    tables, B, q, ranks = cfg["tables"], cfg["B"], cfg["q"], cfg["ranks"]
    rows, D, nnz, nb = int(np.prod(P)), int(np.prod(q)), tables * B * L, tables * B
    torch.manual_seed(1)
    m = ops.TableBatchedTTEmbeddingBag(tables, rows, D, ranks, P, q, weight_dist="uniform", device=dev)
    rs = np.random.RandomState(0)
    idx_h = stream(rs, traffic, nnz, rows)
    keys, counts = np.unique(np.repeat(np.arange(tables), B * L) * rows + idx_h, return_counts=True)
    hot = keys[np.argsort(-counts, kind="stable")[:K_HOT]]
    plain = ttx_infer.TTInferenceBag.from_module(m)
    inf = ttx_infer.TTInferenceBag.from_module(m, hot_indices=[torch.from_numpy(hot[hot // rows == t] % rows) for t in range(tables)])
    idx, off = torch.from_numpy(idx_h).to(dev), torch.arange(0, nnz + 1, L, dtype=torch.int64, device=dev)
    ref, out = plain(idx, off), inf(idx, off)
    hits = int(np.isin(np.repeat(np.arange(tables), B * L) * rows + idx_h, hot).sum())
    print(f"[{name} {traffic}] {nnz} lookups, {len(keys)} distinct keys, K = {inf.hot_rows_count}: hit rate {hits / nnz:.4f}; "
          f"max |with - without| / max |without| = {float((out - ref).abs().max() / ref.abs().max()):.3e}", flush=True)
    fwd = {"without a hot table": captured(lambda: plain(idx, off), CALLS).replay,
           "with the hot table": captured(lambda: inf(idx, off), CALLS).replay}
    for k, (med, lo, hi) in alternate(fwd, windows, steps).items():
        print(f"[{name} {traffic}] forward captured {k:20s} median {med / CALLS * 1e3:8.2f} us/call (min {lo / CALLS * 1e3:.2f}, "
              f"max {hi / CALLS * 1e3:.2f})", flush=True)
    # the launches one by one, each on what the one before it left
    geom = (tables, inf.tt_p_shapes, inf.tt_q_shapes, inf.tt_ranks)
    masked, hit = E.hot_probe_pool(idx, off, tables, rows, inf.hot_keys, inf.hot_rows)
    miss, moff, n_live = E.bags_compact(masked, off, 0, -1)
    _, tab, plan = E.lookup_prologue(miss, moff, *geom, n_dev=n_live)
    mrows = inf._rows_hip(miss, tab, plan)
    stages = {"hot_probe_pool": lambda: E.hot_probe_pool(idx, off, tables, rows, inf.hot_keys, inf.hot_rows),
              "bags_compact": lambda: E.bags_compact(masked, off, 0, -1),
              "lookup_prologue n_dev": lambda: E.lookup_prologue(miss, moff, *geom, n_dev=n_live),
              "tt_rows_bf16 on misses": lambda: inf._rows_hip(miss, tab, plan),
              "bag_sum_pool_add": lambda: E.bag_sum_pool_add(mrows, moff, hit)}
    res = alternate({k: captured(f, CALLS).replay for k, f in stages.items()}, windows, steps)
    moved = 16 * nnz + 8 * (nb + 1) + hits * D * 2 + nb * D * 4
    for k, (med, lo, hi) in res.items():
        us = med / CALLS * 1e3
        extra = f"  {moved / 1e6:.1f} MB by the shapes: {moved / (us * 1e-6) / 1e12:.3f} TB/s" if k == "hot_probe_pool" else ""
        print(f"[{name} {traffic}] launch {k:24s} median {us:8.2f} us (min {lo / CALLS * 1e3:.2f}, max {hi / CALLS * 1e3:.2f}){extra}",
              flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only", default=None, help="one of: " + ", ".join(SHAPES))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    print(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; windows {a.windows}, steps per window {a.steps}, "
          f"{CALLS} calls per captured graph")
    for name, cfg in SHAPES.items():
        for traffic in ("zipf 1.2", "uniform"):
            if a.only in (None, name):
                bench(name, cfg, traffic, a.windows, a.steps)
