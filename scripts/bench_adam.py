"""The fused Adam (OptimType.EXACT_ADAM) on an MI355X.

  kernel   `adam_apply` alone on tensors of the cores' sizes -- cfg2 (3.8 MB), cfg4 (15 MB), 26 tables of cfg2's shape (100 MB):
           microseconds per call and bytes per second (28 bytes per element: 16 read, 12 written), eager (the host's ctypes
           call included) and as a captured graph of CALLS calls replayed (the device's time for the two launches of a call)
  module   the training step at cfg2 (E = 11 M, D = 64, ranks 32, B = 512 x 20 lookups), eager and as a captured round:
           EXACT_ADAM against the same module with sparse=False and torch.optim.Adam on its cores (foreach, and fused=True;
           capturable=True inside the capture), and against the fused-SGD step; alternated in one process, medians of the windows

    python scripts/bench_adam.py [--windows 5] [--steps 1000]
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
import tt_embeddings as E  # noqa: E402
import tt_embeddings_ops as ops  # noqa: E402
import ttx_graph  # noqa: E402

dev = torch.device("cuda:0")
P, B, L, NREQ, CALLS = [200, 220, 250], 512, 20, 4, 20
LR, EPS, BETAS = 1e-3, 1e-8, (0.9, 0.999)
BYTES_PER_ELEMENT = 28  # w, g, m, v read; w, m, v written


def core_numels(tables, q, ranks):
    r = [1] + list(ranks) + [1]
    return [tables * P[t] * r[t] * q[t] * r[t + 1] for t in range(len(q))]


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


def bench_kernel(windows, steps):
    shapes = {"cfg2 cores": core_numels(1, [4, 4, 4], [32, 32]), "cfg4 cores": core_numels(1, [4, 4, 8], [64, 64]),
              "26 x cfg2 cores": core_numels(26, [4, 4, 4], [32, 32])}
    for name, numels in shapes.items():
        ts = [[torch.rand(n, device=dev) * 0.1 for _ in range(4)] for n in numels]
        step = torch.zeros(1, dtype=torch.int64, device=dev)

        def call(_=0):
            E.adam_apply([f[0] for f in ts], [f[1] for f in ts], [f[2] for f in ts], [f[3] for f in ts], step, LR, BETAS, EPS)

        call()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            for _ in range(CALLS):
                call()
        res = alternate({"eager": call, "graph": lambda _: graph.replay()}, windows, steps)
        nbytes = BYTES_PER_ELEMENT * sum(numels)
        for mode, per in (("eager", 1), ("graph", CALLS)):
            med, lo, hi = (x / per * 1e3 for x in res[mode])
            print(f"[kernel] {name:16s} {sum(numels):9d} elements {nbytes / 1e6:7.2f} MB  {mode:5s} median {med:8.2f} us/call "
                  f"(min {lo:.2f}, max {hi:.2f})  {nbytes / med / 1e6:7.3f} TB/s", flush=True)


def bench_module(windows, steps):
    E_, D, q, ranks = int(np.prod(P)), 64, [4, 4, 4], [32, 32]
    rs = np.random.RandomState(0)
    reqs = [(torch.from_numpy(rs.randint(0, E_, size=B * L).astype(np.int64)).to(dev),
             torch.arange(0, B * L + 1, L, dtype=torch.int64, device=dev)) for _ in range(NREQ)]
    grad = torch.rand(B, D, device=dev) * 0.1

    def module(**kw):
        torch.manual_seed(1)
        return ops.TTEmbeddingBag(E_, D, ranks, P, q, learning_rate=LR, eps=EPS, use_cache=False, weight_dist="uniform", device=dev, **kw)

    def external(captured, **okw):
        m = module(sparse=False)
        opt = torch.optim.Adam(list(m.tt_cores), lr=LR, betas=BETAS, eps=EPS, capturable=captured, **okw)

        def step(idx, off):
            opt.zero_grad(set_to_none=True)
            m(idx, off).backward(grad)
            opt.step()
        return step

    def fused(optimizer):
        m = module(sparse=True, optimizer=optimizer)
        return lambda idx, off: m(idx, off).backward(grad)

    def variants(captured):
        v = {"EXACT_ADAM (fused, this library)": fused(ops.OptimType.EXACT_ADAM),
             "sparse=False + torch.optim.Adam(foreach)": external(captured, foreach=True),
             "fused SGD (this library)": fused(ops.OptimType.SGD)}
        try:
            v["sparse=False + torch.optim.Adam(fused=True)"] = external(captured, fused=True)
        except (RuntimeError, TypeError, ValueError) as ex:
            print(f"[module] torch.optim.Adam(fused=True) is not offered here: {ex}")
        return v

    eager = {k: (lambda i, s=s: s(*reqs[i % NREQ])) for k, s in variants(False).items()}
    for k, (med, lo, hi) in alternate(eager, windows, steps).items():
        print(f"[module, eager   ] {k:46s} median {med * 1e3:8.1f} us/step (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
    rounds = {k: ttx_graph.GraphedRound(s, reqs) for k, s in variants(True).items()}
    graphed = {k: (lambda i, r=r: r.replay()) for k, r in rounds.items()}
    for k, (med, lo, hi) in alternate(graphed, windows, max(steps // NREQ, 10)).items():
        print(f"[module, captured] {k:46s} median {med / NREQ * 1e3:8.1f} us/step (min {lo / NREQ * 1e3:.1f}, "
              f"max {hi / NREQ * 1e3:.1f})", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--only", choices=["kernel", "module"], default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    print(f"torch {torch.__version__}, {torch.cuda.get_device_name(0)}; windows {a.windows}, steps per window {a.steps}")
    if a.only in (None, "kernel"):
        bench_kernel(a.windows, a.steps)
    if a.only in (None, "module"):
        bench_module(a.windows, a.steps)
