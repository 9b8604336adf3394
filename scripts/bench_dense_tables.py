"""Dense member tables on the public Criteo-Kaggle cardinalities, D = 64, B = 2048, fused SGD, at one slot per
bag (Criteo's form) and at 20:

  mixed     MixedTTEmbeddingBag(fused=True) with all 26 tables TT against dense_below=10000 (16 tables uncompressed), the two
            alternated in one process, eager and as a captured round (ttx_graph.GraphedRound); medians of five windows
  group     the dense group alone (the 16 tables below 10,000 rows) against 16 nn.EmbeddingBag + torch.optim.SGD
  --profile N steps of the dense group alone and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`; prints
            the bytes a step has to move (computed from the shapes) for the kernel times to be set against

    python scripts/bench_dense_tables.py [--slots 1 20] [--windows 5] [--steps 50]
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/bench_dense_tables.py --profile --slots 20
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "fbtt-embedding_amd"))
import tt_embeddings_ops as ops  # noqa: E402
import ttx_dense  # noqa: E402
import ttx_graph  # noqa: E402
import ttx_mixed  # noqa: E402

CRITEO = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10, 5652, 2173, 4,
          7046547, 18, 15, 286181, 105, 142572]
D, B, BELOW, NREQ = 64, 2048, 10000, 4
dev = torch.device("cuda:0")


def requests(Es, L, seed=0):
    rs = np.random.RandomState(seed)
    reqs = []
    for _ in range(NREQ):
        idx = [torch.from_numpy(rs.randint(0, e, size=B * L).astype(np.int64)).to(dev) for e in Es]
        off = [torch.arange(0, B * L + 1, L, dtype=torch.int64, device=dev) for _ in Es]
        reqs.append((idx, off))
    return reqs


def window(fn, steps):
    """ms per call of fn over one timed window that ends in a device synchronise"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        fn(k)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def alternate(fns, windows, steps):
    """every fn warmed, then `windows` rounds that time each fn once, in turn -> {name: (median, min, max)} ms"""
    for fn in fns.values():
        window(fn, max(4, steps // 5))
    got = {k: [] for k in fns}
    for _ in range(windows):
        for k, fn in fns.items():
            got[k].append(window(fn, steps))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in got.items()}


def show(title, res):
    for k, (med, lo, hi) in res.items():
        print(f"{title:34s} {k:28s} median {med:8.3f} ms/step  (min {lo:.3f}, max {hi:.3f})", flush=True)


def bench_mixed(L, windows, steps):
    reqs = requests(CRITEO, L)
    grads = [torch.rand(B, D, device=dev) * 0.1 for _ in CRITEO]
    kw = dict(sparse=True, optimizer=ops.OptimType.SGD, learning_rate=0.05, weight_dist="uniform", device=dev, fused=True,
              include_last_offset=True)
    mods = {"all TT": ttx_mixed.MixedTTEmbeddingBag(CRITEO, D, [32, 32], **kw),
            f"dense_below={BELOW}": ttx_mixed.MixedTTEmbeddingBag(CRITEO, D, [32, 32], dense_below=BELOW, **kw)}
    steps_of = {k: (lambda idx, off, m=m: torch.autograd.backward(m(idx, off), grads)) for k, m in mods.items()}
    for k, m in mods.items():
        print(f"[mixed, {L} slot(s) per bag] {k}: {len(m.groups)} TT group(s) of {[len(g) for g in m.group_tables]} tables, "
              f"{len(m.dense_groups)} dense group(s) of {[len(g) for g in m.dense_group_tables]} tables", flush=True)
    show(f"mixed eager, {L} slot(s)", alternate({k: (lambda i, s=s: s(*reqs[i % NREQ])) for k, s in steps_of.items()}, windows, steps))
    rounds = {k: ttx_graph.GraphedRound(s, reqs, warmup=2) for k, s in steps_of.items()}
    res = alternate({k: (lambda i, r=r: r.replay()) for k, r in rounds.items()}, windows, max(4, steps // NREQ))
    show(f"mixed captured, {L} slot(s)", {k: tuple(v / NREQ for v in t) for k, t in res.items()})


def small_tables():
    return [e for e in CRITEO if e < BELOW]


def bench_group(L, windows, steps):
    Es = small_tables()
    reqs = requests(Es, L, seed=1)
    merged = [ttx_mixed.merge_bags(i, o, True) for i, o in reqs]
    grad = torch.rand(len(Es), B, D, device=dev) * 0.1
    ours = ttx_dense.DenseTableBatchedEmbeddingBag(Es, D, optimizer=ops.OptimType.SGD, learning_rate=0.05, device=dev)
    fns = {"DenseTableBatchedEmbeddingBag": lambda k: ours(*merged[k % NREQ]).backward(grad)}
    for sparse in (False, True):
        bags = [torch.nn.EmbeddingBag(e, D, mode="sum", sparse=sparse, include_last_offset=True).to(dev) for e in Es]
        opt = torch.optim.SGD([b.weight for b in bags], lr=0.05)

        def step(k, bags=bags, opt=opt):
            idx, off = reqs[k % NREQ]
            opt.zero_grad(set_to_none=True)
            torch.autograd.backward([b(i, o) for b, i, o in zip(bags, idx, off)], list(grad))
            opt.step()
        fns[f"16 nn.EmbeddingBag(sparse={sparse})"] = step
    show(f"dense group alone, {L} slot(s)", alternate(fns, windows, steps))


def profile(L, steps):
    Es = small_tables()
    reqs = requests(Es, L, seed=1)
    merged = [ttx_mixed.merge_bags(i, o, True) for i, o in reqs]
    grad = torch.rand(len(Es), B, D, device=dev) * 0.1
    ours = ttx_dense.DenseTableBatchedEmbeddingBag(Es, D, optimizer=ops.OptimType.SGD, learning_rate=0.05, device=dev)
    for k in range(steps):
        ours(*merged[k % NREQ]).backward(grad)
    torch.cuda.synchronize()
    nb, nnz = len(Es) * B, len(Es) * B * L
    touched = sum(min(e, B * L) for e in Es)  # (an upper bound on the rows a step touches)
    fwd = nnz * 8 + (nb + 1) * 8 + nnz * D * 4 + nb * D * 4      # indices, offsets, one row per lookup, the output
    bwd = nnz * (8 + 16) + nnz * D * 4 + 2 * touched * D * 4     # keys / values in and out, one gradient row per lookup, w read + written
    print(f"[profile] {steps} steps, {len(Es)} tables, {nb} bags, {nnz} lookups per step; bytes a step must move: forward "
          f"{fwd} ({fwd / 6.29e12 * 1e6:.2f} us at 6.29 TB/s), gradient sum + apply {bwd} ({bwd / 6.29e12 * 1e6:.2f} us)", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[1, 20])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--only", choices=["mixed", "group"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    for L in a.slots:
        if a.profile:
            profile(L, a.steps)
            continue
        if a.only != "group":
            bench_mixed(L, a.windows, a.steps)
        if a.only != "mixed":
            bench_group(L, a.windows, a.steps)
