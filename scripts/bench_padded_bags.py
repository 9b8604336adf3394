"""ms/step of a fused-SGD training step (forward + backward) on PADDED bags: what dropping the padding costs.

Workloads: cfg2 (1 table x 512 bags) and cfg5shard (4 tables x 4096 bags), p = [200, 220, 250], q = [4, 4, 4], ranks [32, 32];
bags of 20 live lookups on average padded to L = 40 slots (50 % fill), the padding anywhere in a bag.  Three variants of the
same batches, alternated in one process, eager (one step after another from Python) and replayed (a round of the 10 request
batches captured once with ttx_graph.GraphedRound):

  padded     the 2-D call of a module built with padding_idx: ttx_bags_compact + the n_dev route -- the code under test
  floor      the batch compacted beforehand (outside the timed window), forward(n_dev=): the step with the compaction free
  torch      the compaction as a chain of torch ops (ne / cumsum / where / scatter_ / cat, the table-sharded module's way),
             then forward(n_dev=): what can be written without the kernel

Times are device events around a window of `--steps` steps; every variant of a workload is warmed up first, the windows are
repeated `--repeats` times in turn (padded, floor, torch, padded, ...), the median and the spread (max - min) of the repeats
are reported per variant.

    python scripts/bench_padded_bags.py [--steps 300] [--repeats 5] [--workloads cfg2,cfg5shard] [--json FILE] [--md FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_padded_bags.py --trace      # kernel times, a run of its own

One JSON line per (workload, variant) on stdout; --md writes the table."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fbtt-embedding_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_inputs as G  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_graph  # noqa: E402

P, Q, R, LIVE, SLOTS = [200, 220, 250], [4, 4, 4], [32, 32], 20, 40
WORKLOADS = {"cfg2": (1, 512), "cfg5shard": (4, 4096)}
ITERS = 10
VARIANTS = ("padded", "floor", "torch")
PAD = 0


def padded_requests(seed, nt, B, E_):
    """ITERS batches [nt * B, SLOTS]: gen_inputs' request stream over SLOTS slots per bag, every slot live with probability
    LIVE / SLOTS (bags of LIVE live lookups on average, ragged, the padding anywhere in the bag), PAD elsewhere"""
    rs = np.random.RandomState(seed + 2)
    out = []
    for idx, _ in G.make_requests(seed, ITERS, B, nt, SLOTS, E_):
        idx = np.where(idx == PAD, PAD + 1, idx).reshape(nt * B, SLOTS)
        idx[rs.rand(nt * B, SLOTS) >= LIVE / SLOTS] = PAD
        out.append(idx)
    return out


def torch_compact(idx2d):
    """the padding dropped by torch ops -> (compacted buffer of the same capacity, offsets with the closing entry, n_dev)"""
    N, L = idx2d.shape
    flat = idx2d.reshape(-1)
    cap = flat.numel()
    keep = flat != PAD
    cs = torch.cumsum(keep, 0)
    dest = torch.where(keep, cs - 1, cs.new_full((), cap))
    comp = flat.new_zeros(cap + 1).scatter_(0, dest, flat)[:cap]
    off = torch.cat([cs.new_zeros(1), cs[L - 1::L]])
    return comp, off, cs[-1:].to(torch.int32)


def make_module(nt, dev, padding_idx):
    E_, D = int(np.prod(P)), int(np.prod(Q))
    m = ops.TableBatchedTTEmbeddingBag(nt, E_, D, R, P, Q, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=1e-6,
                                       use_cache=False, weight_dist="uniform", device=dev, padding_idx=padding_idx)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, G.make_cores(1234, nt, P, Q, R, "uniform")):
            dst.copy_(torch.from_numpy(src))
    return m


def window(fn, n):
    """ms per call of fn over n calls, by device events"""
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for k in range(n):
        fn(k)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / n


def measure(workload, steps, warmup, repeats):
    nt, B = WORKLOADS[workload]
    dev = torch.device("cuda", torch.cuda.current_device())
    E_, D = int(np.prod(P)), int(np.prod(Q))
    reqs = [torch.from_numpy(a).to(dev) for a in padded_requests(1235, nt, B, E_)]
    pre = [torch_compact(a) for a in reqs]  # (the floor's batches: compacted outside every timed window)
    fill = float(np.mean([int(c[2].item()) for c in pre])) / reqs[0].numel()
    grad = torch.from_numpy(G.make_grad(1236, nt, B, D)).to(dev)
    mods = {"padded": make_module(nt, dev, PAD), "floor": make_module(nt, dev, None), "torch": make_module(nt, dev, None)}

    def step(variant, k):
        m = mods[variant]
        if variant == "padded":
            out = m(reqs[k])
        elif variant == "floor":
            c, o, n = pre[k]
            out = m(c, o, n_dev=n)
        else:
            c, o, n = torch_compact(reqs[k])
            out = m(c, o, n_dev=n)
        out.backward(grad)

    eager = {v: [] for v in VARIANTS}
    replayed = {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for k in range(warmup):
            step(v, k % ITERS)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in VARIANTS:
            eager[v].append(window(lambda k, v=v: step(v, k % ITERS), steps))
    graphs = {v: ttx_graph.GraphedRound(lambda k, v=v: step(v, k), [(k,) for k in range(ITERS)], warmup=2) for v in VARIANTS}
    rounds = max(1, steps // ITERS)
    for v in VARIANTS:
        graphs[v].replay()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in VARIANTS:
            replayed[v].append(window(lambda k, v=v: graphs[v].replay(), rounds) / ITERS)
    recs = []
    for v in VARIANTS:
        e, r = np.asarray(eager[v]), np.asarray(replayed[v])
        recs.append({"workload": workload, "variant": v, "tables": nt, "bags": nt * B, "slots": nt * B * SLOTS, "fill": round(fill, 3),
                     "eager_ms": round(float(np.median(e)), 4), "eager_spread_ms": round(float(e.max() - e.min()), 4),
                     "replayed_ms": round(float(np.median(r)), 4), "replayed_spread_ms": round(float(r.max() - r.min()), 4),
                     "steps": steps, "repeats": repeats})
    del graphs
    return recs


def trace_run(workloads, steps=100):
    """--trace: only the padded call, eager, `steps` steps per workload in the 2-D form and `steps` in the 1-D + offsets form
    (the route with the offsets gather) -- what to put behind `rocprofv3 --kernel-trace --stats --` for the kernel times"""
    dev = torch.device("cuda", torch.cuda.current_device())
    E_, D = int(np.prod(P)), int(np.prod(Q))
    for wl in workloads:
        nt, B = WORKLOADS[wl]
        reqs = [torch.from_numpy(a).to(dev) for a in padded_requests(1235, nt, B, E_)]
        grad = torch.from_numpy(G.make_grad(1236, nt, B, D)).to(dev)
        m = make_module(nt, dev, PAD)
        for k in range(steps):
            m(reqs[k % ITERS]).backward(grad)
        off = torch.arange(0, reqs[0].numel() + 1, SLOTS, device=dev)
        for k in range(steps):
            m(reqs[k % ITERS].reshape(-1), off).backward(grad)
        torch.cuda.synchronize()


def markdown(recs):
    lines = ["| workload | slots | fill | variant | eager ms/step (spread) | replayed ms/step (spread) |", "|---|---|---|---|---|---|"]
    for r in recs:
        lines.append(f"| {r['workload']} | {r['slots']} | {r['fill']} | {r['variant']} | {r['eager_ms']:.4f} ({r['eager_spread_ms']:.4f}) "
                     f"| {r['replayed_ms']:.4f} ({r['replayed_spread_ms']:.4f}) |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="cfg2,cfg5shard")
    ap.add_argument("--json", default=None, help="also append the lines to this file")
    ap.add_argument("--md", default=None, help="write the table to this file")
    ap.add_argument("--trace", action="store_true", help="run only the padded call, eager (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.trace:
        trace_run(args.workloads.split(","))
        return
    allrecs = []
    for wl in args.workloads.split(","):
        for rec in measure(wl, args.steps, args.warmup, args.repeats):
            allrecs.append(rec)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.json:
                with open(args.json, "a") as f:
                    f.write(line + "\n")
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(allrecs))


if __name__ == "__main__":
    main()
