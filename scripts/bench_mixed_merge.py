"""ms/step of a fused-SGD training step (forward + backward) of MixedTTEmbeddingBag(fused=True): what building the group's
batch costs -- the one-launch merge (`ttx_bags_merge`) against the chain of torch ops the module ran before it had the kernel.

Workloads (D = 64, q = [4, 4, 4], ranks [32, 32], B = 512 bags per table, 20 lookups per bag, uniform indices):
  mixed8    the 8 tables of 4 cardinalities of scripts/bench_mixed.py
  criteo26  26 tables with the cardinalities of the Criteo Kaggle display-advertising set
  ..-padded the same tables, every bag 20 live lookups on average padded to L = 40 slots (2-D input, padding_idx = 0)

Two variants of the same ten batches, alternated in one process, eager (one step after another from Python) and replayed (a
round of the ten batches captured once with ttx_graph.GraphedRound):

  kernel    the module as it is: one `bags_merge` call per group
  chain     the module's `_merge` replaced -- in this script only -- by the torch ops of the earlier forward(): `merge_bags()`
            (a `starts + base` per table, a `full`, two `cat`), and for the padded form a `where` per table in front of it

Times are device events around a window of `--steps` steps; both variants are warmed up first, the windows are repeated
`--repeats` times in turn (kernel, chain, kernel, ...), the median and the spread (max - min) of the repeats are reported.

    python scripts/bench_mixed_merge.py [--steps 200] [--repeats 5] [--workloads mixed8,criteo26,..] [--json FILE] [--md FILE]
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_mixed_merge.py --trace kernel --workloads criteo26 --steps 20
        # launches per step: the difference of the dispatch counts of two such runs (--steps 20 and 60) over 40

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

import tt_embeddings_ops as ops  # noqa: E402
import ttx_graph  # noqa: E402
import ttx_mixed  # noqa: E402

D, Q, R, B, LIVE, SLOTS, PAD = 64, [4, 4, 4], [32, 32], 512, 20, 40, 0
ITERS = 10
VARIANTS = ("kernel", "chain")
_SHAPES8 = {10_000_000: [200, 220, 250], 5_000_000: [160, 180, 200], 1_000_000: [100, 100, 100], 300_000: [64, 70, 72]}
_E8 = [10_000_000, 5_000_000, 1_000_000, 300_000] * 2
CRITEO = [1460, 583, 10131227, 2202608, 305, 24, 12517, 633, 3, 93145, 5683, 8351593, 3194, 27, 14992, 5461306, 10, 5652, 2173,
          4, 7046547, 18, 15, 286181, 105, 142572]
TABLES = {"mixed8": (_E8, [_SHAPES8[e] for e in _E8]), "criteo26": (CRITEO, None)}


def requests(workload, dev):
    """ITERS batches: per table (indices, offsets) -- 1-D indices with B bag starts, or, for a -padded workload, [B, SLOTS]
    indices with every slot live with probability LIVE / SLOTS and offsets None"""
    Es = TABLES[workload.split("-")[0]][0]
    padded = workload.endswith("-padded")
    rs = np.random.RandomState(len(Es))
    out = []
    for _ in range(ITERS):
        idx, off = [], []
        for e in Es:
            if padded:
                i = rs.randint(1, e, size=(B, SLOTS)).astype(np.int64)  # (PAD = 0 is no live value)
                i[rs.rand(B, SLOTS) >= LIVE / SLOTS] = PAD
                idx.append(torch.from_numpy(i).to(dev))
                off.append(None)
            else:
                idx.append(torch.from_numpy(rs.randint(0, e, size=B * LIVE).astype(np.int64)).to(dev))
                off.append(torch.arange(0, B * LIVE, LIVE, dtype=torch.int64, device=dev))
        out.append((idx, off))
    return out


def make_module(workload, dev):
    Es, ps = TABLES[workload.split("-")[0]]
    torch.manual_seed(7)
    return ttx_mixed.MixedTTEmbeddingBag(Es, D, R, ps, Q, sparse=True, optimizer=ops.OptimType.SGD, learning_rate=1e-6,
                                         weight_dist="uniform", device=dev, include_last_offset=False, fused=True,
                                         padding_idx=PAD if workload.endswith("-padded") else None)


_starts = {}


def chain_merge(self, tables, indices, offsets, per_sample_weights):
    """`MixedTTEmbeddingBag._merge` as torch ops: what forward() ran before the kernel (1-D inputs: exactly that); the 2-D form
    is flattened against bag starts kept from call to call, the padding rewritten with one `where` per padded table"""
    idx, off = [], []
    for k in tables:
        i, o = indices[k], offsets[k]
        if o is None:
            o = _starts.get(i.shape)
            if o is None:
                o = _starts[i.shape] = torch.arange(0, i.numel(), i.size(1), dtype=torch.int64, device=i.device)
            i = i.reshape(-1)
        v = self.padding_idx[k]
        idx.append(i if v is None else torch.where(i == v, ttx_mixed.PAD_SENTINEL, i))
        off.append(o)
    mi, mo = ttx_mixed.merge_bags(idx, off, self.include_last_offset)
    return mi, mo, None


def window(fn, n):
    """ms per call of fn over n calls, by device events"""
    beg, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    beg.record()
    for k in range(n):
        fn(k)
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) / n


def stepper(workload, dev):
    reqs = requests(workload, dev)
    mods = {v: make_module(workload, dev) for v in VARIANTS}
    mods["chain"].load_state_dict(mods["kernel"].state_dict())
    mods["chain"]._merge = chain_merge.__get__(mods["chain"])
    grads = [torch.rand(B, D, device=dev) * 0.1 for _ in mods["kernel"].num_embeddings]

    def step(variant, k):
        torch.autograd.backward(mods[variant](*reqs[k]), grads)

    # the two variants must train the same tables to the same bits
    outs = {v: torch.stack([o.detach() for o in mods[v](*reqs[0])]) for v in VARIANTS}
    assert torch.equal(outs["kernel"], outs["chain"]), "the kernel merge and the torch chain disagree"
    return step, mods, reqs


def measure(workload, steps, warmup, repeats):
    dev = torch.device("cuda", torch.cuda.current_device())
    step, mods, reqs = stepper(workload, dev)
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
    nt = len(mods["kernel"].num_embeddings)
    slots = sum(int(i.numel()) for i in reqs[0][0])
    for v in VARIANTS:
        e, r = np.asarray(eager[v]), np.asarray(replayed[v])
        recs.append({"workload": workload, "variant": v, "tables": nt, "groups": len(mods[v].groups), "slots": slots,
                     "eager_ms": round(float(np.median(e)), 4), "eager_spread_ms": round(float(e.max() - e.min()), 4),
                     "replayed_ms": round(float(np.median(r)), 4), "replayed_spread_ms": round(float(r.max() - r.min()), 4),
                     "steps": steps, "repeats": repeats})
    del graphs
    return recs


def trace_run(variant, workloads, steps):
    """--trace: `steps` eager steps of ONE variant per workload and nothing else that depends on `steps`: two runs behind
    `rocprofv3 --kernel-trace --stats --` that differ in --steps differ by that many steps' dispatches"""
    dev = torch.device("cuda", torch.cuda.current_device())
    for wl in workloads:
        step, _, _ = stepper(wl, dev)
        for k in range(steps):
            step(variant, k % ITERS)
        torch.cuda.synchronize()


def markdown(recs):
    lines = ["| workload | tables | slots | variant | eager ms/step (spread) | replayed ms/step (spread) |", "|---|---|---|---|---|---|"]
    for r in recs:
        lines.append(f"| {r['workload']} | {r['tables']} | {r['slots']} | {r['variant']} | {r['eager_ms']:.4f} ({r['eager_spread_ms']:.4f}) "
                     f"| {r['replayed_ms']:.4f} ({r['replayed_spread_ms']:.4f}) |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--workloads", default="mixed8,criteo26,mixed8-padded,criteo26-padded")
    ap.add_argument("--json", default=None, help="also append the lines to this file")
    ap.add_argument("--md", default=None, help="write the table to this file")
    ap.add_argument("--trace", choices=VARIANTS, default=None, help="run only this variant, eager (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    if args.trace:
        trace_run(args.trace, args.workloads.split(","), args.steps)
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
