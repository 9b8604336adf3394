"""ms/step of a fused-SGD training step (forward + backward) in each pooling mode -- sum, mean, max -- at the benchmark's
shapes: cfg2 (one table, 512 bags of 20 lookups = 10,240 lookups) and cfg5shard (4 tables x 4096 bags x 20 = 327,680 lookups),
p = [200, 220, 250], q = [4, 4, 4], ranks [32, 32].  Eager (one step after another from Python) and replayed (a round of the 10
request batches captured once with ttx_graph.GraphedRound, then replayed).  No cache (max mode has none), so every mode runs
the same contraction work.

    python scripts/bench_pooling_modes.py [--steps 200] [--workloads cfg2,cfg5shard] [--modes sum,mean,max] [--json FILE]

One JSON line per (workload, mode) on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "fbtt-embedding_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import gen_inputs as G  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_graph  # noqa: E402

P, Q, R, L = [200, 220, 250], [4, 4, 4], [32, 32], 20
WORKLOADS = {"cfg2": (1, 512), "cfg5shard": (4, 4096)}
ITERS = 10


def measure(workload, mode, steps, warmup):
    nt, B = WORKLOADS[workload]
    dev = torch.device("cuda", torch.cuda.current_device())
    E_, D = int(np.prod(P)), int(np.prod(Q))
    m = ops.TableBatchedTTEmbeddingBag(nt, E_, D, R, P, Q, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=1e-6,
                                       use_cache=False, weight_dist="uniform", device=dev, mode=mode)
    with torch.no_grad():
        for dst, src in zip(m.tt_cores, G.make_cores(1234, nt, P, Q, R, "uniform")):
            dst.copy_(torch.from_numpy(src))
    reqs = [(torch.from_numpy(i).to(dev), torch.from_numpy(o).to(dev)) for i, o in G.make_requests(1235, ITERS, B, nt, L, E_)]
    grad = torch.from_numpy(G.make_grad(1236, nt, B, D)).to(dev)

    def step(i, o):
        m(i, o).backward(grad)

    for k in range(warmup):
        step(*reqs[k % ITERS])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        step(*reqs[k % ITERS])
    torch.cuda.synchronize()
    eager = (time.perf_counter() - t0) * 1e3 / steps
    graph = ttx_graph.GraphedRound(step, reqs, warmup=2)
    rounds = max(1, steps // ITERS)
    graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(rounds):
        graph.replay()
    torch.cuda.synchronize()
    replayed = (time.perf_counter() - t0) * 1e3 / (rounds * ITERS)
    del graph
    return {"workload": workload, "mode": mode, "lookups": nt * B * L, "tables": nt, "bags": nt * B, "D": D,
            "eager_ms": round(eager, 4), "replayed_ms": round(replayed, 4), "steps": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workloads", default="cfg2,cfg5shard")
    ap.add_argument("--modes", default="sum,mean,max")
    ap.add_argument("--json", default=None, help="also append the lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    for wl in args.workloads.split(","):
        for mode in args.modes.split(","):
            rec = measure(wl, mode, args.steps, args.warmup)
            line = json.dumps(rec)
            print(line, flush=True)
            if args.json:
                with open(args.json, "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
