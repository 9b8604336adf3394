"""ms/step of a fused-SGD training step (forward + backward) of an UNPOOLED lookup: TTEmbedding against the way to the same
result without it, TTEmbeddingBag with one bag per lookup.

Workloads (one table each):
  cfg2-10k / cfg2-327k   the benchmark geometry (BASELINE.json cfg2's table: p = [200, 220, 250], q = [4, 4, 4], ranks 32) at
                         10,240 and 327,680 lookups
  token-4k / token-32k   a token-like table: E = 50,257, D = 512 (q = [8, 8, 8], ranks [32, 32]: the core-0 row split), 8 x 512
                         and 64 x 512 positions
each at 0 % and 30 % padding.  Two variants of the same batches, alternated in one process, eager (one step after another from
Python) and replayed (the step captured once with ttx_graph.GraphedStep, the batches copied into its static buffers):

  embedding   TTEmbedding(padding_idx=)(indices [rows, cols]) -> [rows, cols, D]: the code under test
  bags        TTEmbeddingBag(use_cache=False, padding_idx=)(indices [N, 1]) -> [N, D]: N bags of one slot (0 % padding: the 1-D
              call with offsets arange(N + 1), no padding_idx on either module)

Times are device events around a window of `--steps` steps; both variants are warmed up first, the windows are repeated
`--repeats` times in turn (embedding, bags, embedding, ...), the median and the spread (max - min) of the repeats are reported.

    python scripts/bench_unpooled.py [--steps 200] [--repeats 5] [--workloads cfg2-10k,token-4k] [--json FILE] [--md FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_unpooled.py --trace      # kernel times, a run of its own

One JSON line per (workload, padding, variant) on stdout; --md writes the table.

--cache: the same comparison with a LIVE row cache (DESIGN.md 4.12 "with the row cache"), no padding, a Zipf(1.2) index stream:

  embedding   TTEmbedding(use_cache=True): partition, plan of the misses, contraction, rows_place / rows_pick, cache rows' update
  bags        TTEmbeddingBag(use_cache=True)(indices, arange(N + 1)): one bag per position through the cache-live C++ node

on the token-like table and on cfg2's table at 4,096 and 32,768 positions (CACHE_WORKLOADS).  Both modules count the same
warm-up batches of the stream and populate before anything is timed; the hit share of the timed batches is reported.

    python scripts/bench_unpooled.py --cache [--steps 200] [--repeats 5] [--workloads token-4k,cfg2-32k] [--json FILE] [--md FILE]"""
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

import tt_embeddings_ops as ops  # noqa: E402
import ttx_graph  # noqa: E402

# name -> (num_embeddings, D, p, q, ranks, index shape)
WORKLOADS = {
    "cfg2-10k": (200 * 220 * 250, 64, [200, 220, 250], [4, 4, 4], [32, 32], (20, 512)),
    "cfg2-327k": (200 * 220 * 250, 64, [200, 220, 250], [4, 4, 4], [32, 32], (640, 512)),
    "token-4k": (50257, 512, None, [8, 8, 8], [32, 32], (8, 512)),
    "token-32k": (50257, 512, None, [8, 8, 8], [32, 32], (64, 512)),
}
# --cache: name -> (num_embeddings, D, p, q, ranks, index shape, cache rows, hash table slots)
CACHE_WORKLOADS = {
    "token-4k": (50257, 512, None, [8, 8, 8], [32, 32], (8, 512), 4096, 1 << 17),
    "token-32k": (50257, 512, None, [8, 8, 8], [32, 32], (64, 512), 4096, 1 << 17),
    "cfg2-4k": (200 * 220 * 250, 64, [200, 220, 250], [4, 4, 4], [32, 32], (8, 512), 16384, 1 << 20),
    "cfg2-32k": (200 * 220 * 250, 64, [200, 220, 250], [4, 4, 4], [32, 32], (64, 512), 16384, 1 << 20),
}
ZIPF_ALPHA = 1.2
ITERS = 4
VARIANTS = ("embedding", "bags")
SHARES = (0.0, 0.3)
PAD = 0


def requests(seed, shape, E_, share):
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(ITERS):
        idx = rs.randint(1, E_, size=shape).astype(np.int64)
        if share > 0:
            idx[rs.rand(*shape) < share] = PAD
        out.append(idx)
    return out


def make_modules(wl, dev, padding_idx):
    E_, D, p, q, r, _ = WORKLOADS[wl]
    kw = dict(optimizer=ops.OptimType.SGD, learning_rate=1e-6, sparse=True, weight_dist="uniform", device=dev, padding_idx=padding_idx)
    torch.manual_seed(1234)
    emb = ops.TTEmbedding(E_, D, r, p, q, **kw)
    bag = ops.TTEmbeddingBag(E_, D, r, p, q, use_cache=False, **kw)
    with torch.no_grad():
        for dst, src in zip(bag.tt_cores, emb.tt_cores):
            dst.copy_(src)
    return {"embedding": emb, "bags": bag}


def window(fn, n):
    """ms per call of fn over n calls, by device events"""
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for k in range(n):
        fn(k)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / n


def measure(wl, share, steps, warmup, repeats):
    E_, D, _, _, _, shape = WORKLOADS[wl]
    N = int(np.prod(shape))
    dev = torch.device("cuda", torch.cuda.current_device())
    reqs = [torch.from_numpy(a).to(dev) for a in requests(1235, shape, E_, share)]
    grad = (torch.rand(shape + (D,), device=dev) * 0.1).contiguous()
    mods = make_modules(wl, dev, PAD if share > 0 else None)
    off = torch.arange(N + 1, device=dev)

    def step(variant, idx, g):
        m = mods[variant]
        if variant == "embedding":
            out = m(idx)
        elif share > 0:
            out = m(idx.reshape(N, 1))
        else:
            out = m(idx.reshape(-1), off)
        out.backward(g.view(out.shape))

    eager = {v: [] for v in VARIANTS}
    replayed = {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for k in range(warmup):
            step(v, reqs[k % ITERS], grad)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in VARIANTS:
            eager[v].append(window(lambda k, v=v: step(v, reqs[k % ITERS], grad), steps))
    # (the bag module's padded route reads the live count back when the table takes part lookups, q0 > 4: nothing to replay there)
    capturable = [v for v in VARIANTS if not (v == "bags" and share > 0 and getattr(mods[v], "_split0", 0) > 1)]
    graphs = {v: ttx_graph.GraphedStep(lambda i, g, v=v: step(v, i, g), (reqs[0], grad), warmup=2) for v in capturable}
    for v in capturable:
        graphs[v](reqs[0], grad)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in capturable:
            replayed[v].append(window(lambda k, v=v: graphs[v](reqs[k % ITERS], grad), steps))
    recs = []
    for v in VARIANTS:
        e, r = np.asarray(eager[v]), np.asarray(replayed[v])
        recs.append({"workload": wl, "positions": N, "D": D, "padding": share, "variant": v, "split0": int(getattr(mods[v], "_split0", 0)),
                     "eager_ms": round(float(np.median(e)), 4), "eager_spread_ms": round(float(e.max() - e.min()), 4),
                     "replayed_ms": round(float(np.median(r)), 4) if r.size else None,
                     "replayed_spread_ms": round(float(r.max() - r.min()), 4) if r.size else None,
                     "steps": steps, "repeats": repeats})
    del graphs
    return recs


def zipf_requests(seed, shape, E_, count):
    """`count` batches of a Zipf(ZIPF_ALPHA) stream over E_ keys (the ranks scattered over the key space by a fixed multiplier)"""
    rs = np.random.RandomState(seed)
    return [(((rs.zipf(ZIPF_ALPHA, size=shape).astype(np.int64) - 1) % E_) * 2654435761 % E_).astype(np.int64) for _ in range(count)]


def measure_cache(wl, steps, warmup, repeats):
    E_, D, p, q, r, shape, cache_size, hashtbl_size = CACHE_WORKLOADS[wl]
    N = int(np.prod(shape))
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = zipf_requests(1236, shape, E_, 16 + ITERS)
    warm, reqs = [torch.from_numpy(a).to(dev) for a in stream[:16]], [torch.from_numpy(a).to(dev) for a in stream[16:]]
    grad = (torch.rand(shape + (D,), device=dev) * 0.1).contiguous()
    off = torch.arange(N + 1, device=dev)
    kw = dict(optimizer=ops.OptimType.SGD, learning_rate=1e-6, sparse=True, weight_dist="uniform", device=dev, use_cache=True,
              cache_size=cache_size, hashtbl_size=hashtbl_size)
    torch.manual_seed(1234)
    mods = {"embedding": ops.TTEmbedding(E_, D, r, p, q, **kw), "bags": ops.TTEmbeddingBag(E_, D, r, p, q, **kw)}
    with torch.no_grad():
        for dst, src in zip(mods["bags"].tt_cores, mods["embedding"].tt_cores):
            dst.copy_(src)

    def step(variant, idx, g):
        m = mods[variant]
        out = m(idx) if variant == "embedding" else m(idx.reshape(-1), off)
        out.backward(g.view(out.shape))

    with torch.no_grad():
        for v in VARIANTS:
            for b in warm:
                step_out = mods[v](b) if v == "embedding" else mods[v](b.reshape(-1), off)
                del step_out
            mods[v].cache_populate()
    m = mods["embedding"]
    keys = m.hashtbl[m.cache_state >= 0].cpu().numpy()
    hit_share = float(np.mean([np.isin(a, keys).mean() for a in stream[16:]]))
    eager = {v: [] for v in VARIANTS}
    replayed = {v: [] for v in VARIANTS}
    for v in VARIANTS:
        for k in range(warmup):
            step(v, reqs[k % ITERS], grad)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in VARIANTS:
            eager[v].append(window(lambda k, v=v: step(v, reqs[k % ITERS], grad), steps))
    graphs = {v: ttx_graph.GraphedStep(lambda i, g, v=v: step(v, i, g), (reqs[0], grad), warmup=2) for v in VARIANTS}
    for v in VARIANTS:
        graphs[v](reqs[0], grad)
    torch.cuda.synchronize()
    for _ in range(repeats):
        for v in VARIANTS:
            replayed[v].append(window(lambda k, v=v: graphs[v](reqs[k % ITERS], grad), steps))
    recs = []
    for v in VARIANTS:
        e, rp = np.asarray(eager[v]), np.asarray(replayed[v])
        recs.append({"workload": wl, "cache": True, "positions": N, "D": D, "padding": 0.0, "hit_share": round(hit_share, 3),
                     "variant": v, "split0": int(getattr(mods[v], "_split0", 0)),
                     "eager_ms": round(float(np.median(e)), 4), "eager_spread_ms": round(float(e.max() - e.min()), 4),
                     "replayed_ms": round(float(np.median(rp)), 4), "replayed_spread_ms": round(float(rp.max() - rp.min()), 4),
                     "steps": steps, "repeats": repeats})
    del graphs
    return recs


def trace_run(workloads, steps=50):
    """--trace: only TTEmbedding with 30 % padding, eager, `steps` steps per workload -- what to put behind
    `rocprofv3 --kernel-trace --stats --` for the kernel times of rows_expand* / rows_collect*"""
    dev = torch.device("cuda", torch.cuda.current_device())
    for wl in workloads:
        E_, D, _, _, _, shape = WORKLOADS[wl]
        reqs = [torch.from_numpy(a).to(dev) for a in requests(1235, shape, E_, 0.3)]
        grad = (torch.rand(shape + (D,), device=dev) * 0.1).contiguous()
        m = make_modules(wl, dev, PAD)["embedding"]
        for k in range(steps):
            m(reqs[k % ITERS]).backward(grad)
        torch.cuda.synchronize()


def markdown(recs):
    cache = any(r.get("cache") for r in recs)
    third = "hit share" if cache else "padding"
    lines = [f"| workload | positions | D | {third} | variant | eager ms/step (spread) | replayed ms/step (spread) |", "|---|---|---|---|---|---|---|"]
    for r in recs:
        rep = "not capturable" if r["replayed_ms"] is None else f"{r['replayed_ms']:.4f} ({r['replayed_spread_ms']:.4f})"
        share = r["hit_share"] if cache else r["padding"]
        lines.append(f"| {r['workload']} | {r['positions']} | {r['D']} | {share:.0%} | {r['variant']} | {r['eager_ms']:.4f} ({r['eager_spread_ms']:.4f}) "
                     f"| {rep} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default=None, help="comma-separated; default: all of WORKLOADS (--cache: of CACHE_WORKLOADS)")
    ap.add_argument("--cache", action="store_true", help="the cache-live comparison on a Zipf stream (CACHE_WORKLOADS)")
    ap.add_argument("--json", default=None, help="also append the lines to this file")
    ap.add_argument("--md", default=None, help="write the table to this file")
    ap.add_argument("--trace", action="store_true", help="run only TTEmbedding with padding, eager (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    workloads = (args.workloads or ",".join(CACHE_WORKLOADS if args.cache else WORKLOADS)).split(",")
    if args.trace:
        trace_run(workloads)
        return
    allrecs = []
    for wl in workloads:
        for share in ((None,) if args.cache else SHARES):
            for rec in (measure_cache(wl, args.steps, args.warmup, args.repeats) if args.cache
                        else measure(wl, share, args.steps, args.warmup, args.repeats)):
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
