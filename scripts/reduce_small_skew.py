"""reduce + apply duration on uniform and skewed batches of the cfg2 geometry (SGD), small kernel against reduce_apply_kernel
(ttx_debug_skip bit 21), both through the test library in one process; after scripts/reduce_small.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fbtt-embedding_amd"))
import tt_embeddings as E

dev = torch.device("cuda:0")
p, q, r = [200, 220, 250], [4, 4, 4], [1, 32, 32, 1]
E_, D, B = 200 * 220 * 250, 64, 512
Lt = torch.tensor([220 * 250, 250, 1], dtype=torch.int64, device=dev)
cores = [torch.randn(1, p[k], r[k] * q[k] * r[k + 1], device=dev) * 0.1 for k in range(3)]
rs = np.random.RandomState(0)
PROF = {"bwd": 1, "reduce": 2}


def zipf(n, a=1.2):  # rank == index, sampled from the normalised 1/k^a over the table's rows
    w = 1.0 / np.arange(1, E_ + 1, dtype=np.float64) ** a
    cdf = np.cumsum(w)
    return np.searchsorted(cdf, rs.rand(n) * cdf[-1]).astype(np.int64)


CASES = (("uniform", 10240, lambda n: rs.randint(0, E_, size=n)), ("zipf 1.2", 10240, zipf),
         ("one row", 16384, lambda n: np.full(n, 123456)), ("one row", 10240, lambda n: np.full(n, 123456)))
for label, nnz, gen in CASES:
    idx_np = gen(nnz).astype(np.int64)
    top = np.bincount(idx_np % 1000003).max()
    idx = torch.from_numpy(idx_np).to(dev)
    rowidx = torch.from_numpy(np.sort(rs.randint(0, B, size=nnz)).astype(np.int64)).to(dev)
    tableidx = torch.zeros(nnz, dtype=torch.int64, device=dev)
    d_out = torch.randn(1, B, D, device=dev)
    for knob, name in ((0, "small"), (1 << 21, "full"), (0, "small"), (1 << 21, "full")):
        if knob:
            E.debug_skip(knob)
        try:
            with E.test_library():
                plan = E.make_plan(1, p, q, r, nnz, idx, tableidx, rowidx)
                for it in range(5):
                    E.tt_sgd_backward(1000, D, 1e-6, p, q, r, Lt, nnz, idx, rowidx, tableidx, d_out, cores, plan=plan)
                torch.cuda.synchronize()
                route = E.debug_reduce_route()
                E.profile_enable(0xff)
                E.profile_reset()
                for it in range(40):
                    E.tt_sgd_backward(1000, D, 1e-6, p, q, r, Lt, nnz, idx, rowidx, tableidx, d_out, cores, plan=plan)
                torch.cuda.synchronize()
                out = {k: E.profile_read(w) for k, w in PROF.items()}
                E.profile_enable(0)
        finally:
            if knob:
                E.debug_skip(0)
        print(f"{label} nnz={nnz} (most frequent row: {top} lookups) {name} (route {route}):",
              {k: round(ms / max(n, 1) * 1e3, 2) for k, (n, ms) in out.items() if n}, "us (HIP events)", flush=True)
