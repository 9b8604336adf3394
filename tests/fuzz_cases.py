"""Randomised parity sweeps, GPU (libttx through the C ABI shim) vs the CPU oracle.  TEST INFRASTRUCTURE.

run_plan_cases: geometry (T, q, ranks, p up to 3000), table count, batch, ragged / empty bags and a
70 %-on-three-indices skew drawn at random so that every plan route (tiny / single launch / wave units / wide
digit / table groups / multi-pass), the generic kernels' block walk of core 1 (small LDS budgets), per-table row factors (ttx_geom::p_tables) and the module's route
(ttx_lookup_prologue) are hit; forward + dense gradients, and -- tables of one row factoring -- fused SGD and fused Adagrad from a
non-zero state, then forward and both fused backwards once more with per_sample_weights against the weighted float64 reference.
run_cache_cases: the cache-live prologue (offsets -> bag rows, cache lookup, stable partition: bit-exact) and the
cache gather / SGD scatter.

A fixed-seed slice of each runs under `-m gpu` (tests/test_fuzz_gpu.py); scripts/fuzz_plan.py and
scripts/fuzz_cache.py run them for a time budget."""
import ctypes as C
import time

import numpy as np
import torch

import gen_inputs as G
import oracle_lib as O
import plan_ref as PR
import tt_ref64 as R
from util import ATOL_SCALE, RTOL, assert_adagrad_close, assert_close

dev = torch.device("cuda:0")


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def run_plan_cases(seed=0, max_cases=None, budget=None):
    """-> (cases run, {route: count})"""
    import tt_embeddings as E

    rs = np.random.RandomState(seed)
    t0, n, routes = time.time(), 0, {}
    while (budget is None or time.time() - t0 < budget) and (max_cases is None or n < max_cases):
        T = int(rs.choice([2, 3, 3, 3, 4]))
        tables = int(rs.choice([1, 1, 2, 3, 5, 9, 20, 40]))
        spec = T == 3 and rs.rand() < 0.4
        if spec:
            # the shape-specialised kernels' families: q0 = 4 / 2, q1 = 2 / 4 / 8 (ttx_tt_spec.inc)
            q = [[4, 4, 4], [4, 4, 8], [2, 4, 4], [2, 2, 4], [4, 8, 8]][int(rs.randint(0, 5))]
            r = [1] + [int(rs.choice([16, 32]))] * 2 + [1]
        else:
            q = [int(rs.randint(1, 5)) for _ in range(T)]
            r = [1] + [int(rs.randint(1, 9)) for _ in range(T - 1)] + [1]
            if rs.rand() < 0.3:  # larger ranks: K blocks of core 1 (r1 > 32) once the LDS budget below is small
                r = [1] + [int(rs.randint(1, 72)) for _ in range(T - 1)] + [1]
        # the generic kernels' block walk (K blocks x column passes of a core_1 slice, csrc/ttx_tt_generic.inc): a small
        # LDS budget drives these small shapes through it
        lds_kb = 0 if spec else int(rs.choice([0, 0, 12, 16, 24, 40]))
        pmax = int(rs.choice([6, 40, 300, 700, 3000]))
        p = [int(rs.randint(2, pmax + 1)) for _ in range(T)]
        if np.prod(np.array(p, dtype=np.float64)) * 1.0 > 2e12:
            continue
        E_ = int(np.prod(np.array(p, dtype=np.int64)))
        D = int(np.prod(q))
        B = int(rs.choice([1, 7, 64, 300, 1500]))
        pf = int(rs.choice([1, 3, 10, 40]))
        nnz_est = tables * B * pf
        if nnz_est > 150000:
            continue
        lens = rs.randint(0, 2 * pf + 1, size=tables * B)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        nnz = int(off[-1])
        if nnz == 0:
            continue
        idx = rs.randint(0, E_, size=nnz).astype(np.int64)
        if rs.rand() < 0.3:
            hot = rs.randint(0, E_, size=3)
            idx = np.where(rs.rand(nnz) < 0.7, hot[rs.randint(0, 3, size=nnz)], idx).astype(np.int64)
        d_out = G.make_grad(int(rs.randint(1 << 30)), tables, B, D)
        E.debug_lds_budget(lds_kb * 1024)
        walk = E.debug_tiles(tables, p, q, r)
        if not spec and walk["MC"] == 0:  # (nothing fits that budget)
            E.debug_lds_budget(0)
            walk = E.debug_tiles(tables, p, q, r)
        if walk["ncp"] * walk["nkb"] > 1:
            routes["block-walk"] = routes.get("block-walk", 0) + 1
        if tables > 1 and rs.rand() < 0.35:
            # tables of different row factors (ttx_geom::p_tables): the oracle does every table on its own
            ps = [[int(rs.randint(2, pmax + 1)) for _ in range(T)] for _ in range(tables)]
            Es = [int(np.prod(np.array(pk, dtype=np.int64))) for pk in ps]
            if max(Es) > 2e12:
                continue
            bounds = off[::B]
            idx = np.concatenate([rs.randint(0, Es[k], size=int(bounds[k + 1] - bounds[k])) for k in range(tables)]).astype(np.int64)
            tcores = [G.make_cores(int(rs.randint(1 << 30)), 1, ps[k], q, r[1:-1], "signed") for k in range(tables)]
            gc = [t(np.concatenate([tcores[k][c_] for k in range(tables)], axis=1)) for c_ in range(T)]
            Lt = torch.zeros(T, dtype=torch.int64, device=dev)
            if rs.rand() < 0.5:  # the module's route: offsets -> rows + plan (table groups when the slice ids need them)
                ri, ti, plan = E.lookup_prologue(t(idx), t(off), tables, ps, q, r)
                routes["prologue"] = routes.get("prologue", 0) + 1
            else:
                ri, ti = E.preprocess_indices_sync(t(idx), t(off), tables, True, torch.empty(0, dtype=torch.int64, device=dev),
                                                   torch.empty(0, dtype=torch.int32, device=dev))[1:3]
                plan = E.make_plan(tables, ps, q, r, nnz, t(idx), ti, ri)
            out = E.tt_forward(1000, tables, B, D, ps, q, r, Lt, nnz, t(idx), ri, ti, gc, plan=plan)
            grads = E.tt_dense_backward(1000, D, ps, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gc, plan=plan)
            what = f"case {n} (mixed): T={T} p={ps} q={q} r={r} B={B} nnz={nnz}"
            tol = dict(rtol=2e-5, atol_scale=4e-6)  # (measured worst: 0.8x the default bound, profiles/r05_tolerances.md)
            gsplit = [torch.split(grads[c_][0], [pk[c_] for pk in ps], dim=0) for c_ in range(T)]
            for k in range(tables):
                gk = O.make_geom(1, ps[k], q, r)
                ik, ok = idx[bounds[k]:bounds[k + 1]], off[k * B:(k + 1) * B + 1] - bounds[k]
                rk, tk = O.rowidx_from_offsets(ok, 1)
                assert_close(out[k].cpu().numpy(), O.tt_forward(gk, B, D, ik, rk, tk, tcores[k])[0], what + f" out table {k}", **tol)
                rg = O.tt_backward(gk, O.OPTIM_DENSE, B, D, 0, 0, ik, rk, tk, d_out[k:k + 1], [x.copy() for x in tcores[k]])
                for c_ in range(T):
                    assert_close(gsplit[c_][k].cpu().numpy(), rg[c_][0], what + f" grad{c_} table {k}", **tol)
            routes["mixed"] = routes.get("mixed", 0) + 1
            n += 1
            E.debug_lds_budget(0)
            continue
        cores = G.make_cores(int(rs.randint(1 << 30)), tables, p, q, r[1:-1], "signed")
        c = dict(tables=tables, T=T, p=p, q=q, r=r, B=B, D=D)
        g = O.make_geom(tables, p, q, r)
        rowidx, tableidx = O.rowidx_from_offsets(off, tables)
        ref_out = O.tt_forward(g, B, D, idx, rowidx, tableidx, cores)
        ref_g = O.tt_backward(g, O.OPTIM_DENSE, B, D, 0, 0, idx, rowidx, tableidx, d_out, [x.copy() for x in cores])
        Lt = t(np.array([int(np.prod(p[k + 1:])) for k in range(T)], dtype=np.int64))
        gc = [t(x) for x in cores]
        by_prologue = tables > 1 and rs.rand() < 0.5
        if by_prologue:
            ri, ti, plan = E.lookup_prologue(t(idx), t(off), tables, p, q, r)
            routes["prologue"] = routes.get("prologue", 0) + 1
        else:
            ri, ti = E.preprocess_indices_sync(t(idx), t(off), tables, True, torch.empty(0, dtype=torch.int64, device=dev),
                                               torch.empty(0, dtype=torch.int32, device=dev))[1:3]
            plan = E.make_plan(tables, p, q, r, nnz, t(idx), ti, ri)
        out = E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, t(idx), ri, ti, gc, plan=plan)
        grads = E.tt_dense_backward(1000, D, p, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gc, plan=plan)
        what = f"case {n}: T={T} tables={tables} p={p} q={q} r={r} B={B} nnz={nnz} walk={walk}"
        tol = dict(rtol=5e-5, atol_scale=1e-5)  # (hot slices: thousands of terms in an order of their own; measured worst: 2.25x the default bound, profiles/r08_tolerances.md)
        assert_close(out.cpu().numpy(), ref_out, what + " out", **tol)
        for k in range(T):
            assert_close(grads[k].cpu().numpy(), ref_g[k], what + f" grad{k}", **tol)
        # the fused optimizers on the same route: SGD, and Adagrad from a NON-ZERO state (s = s0 + g^2 -- a zero state cannot tell that
        # from s = g^2), against the oracle at the case's tolerance.  (Draws from a stream of their own: the cases above stay what
        # they were.)
        rs2 = np.random.RandomState([seed, n, 78])
        lr, eps = float(rs2.choice([0.1, 0.02])), float(rs2.choice([1e-4, 1e-2]))
        state0 = [(rs2.rand(*x.shape) * 2.0 * max(float((gk * gk).max()), 1e-12)).astype(np.float32) for x, gk in zip(cores, ref_g)]
        ref_w = [x.copy() for x in cores]
        O.tt_backward(g, O.OPTIM_SGD, B, D, lr, 0, idx, rowidx, tableidx, d_out, ref_w)
        gw = [t(x) for x in cores]
        E.tt_sgd_backward(1000, D, lr, p, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gw, plan=plan)
        for k in range(T):
            assert_close(gw[k].cpu().numpy(), ref_w[k], what + f" sgd core{k} lr={lr}", **tol)
        ref_w, ref_s = [x.copy() for x in cores], [x.copy() for x in state0]
        O.tt_backward(g, O.OPTIM_ADAGRAD, B, D, lr, eps, idx, rowidx, tableidx, d_out, ref_w, ref_s)
        gw, gs = [t(x) for x in cores], [t(x) for x in state0]
        E.tt_adagrad_backward(1000, D, lr, eps, p, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gs, gw, plan=plan)
        for k in range(T):
            assert_close(gs[k].cpu().numpy(), ref_s[k], what + f" adagrad state{k}", **tol)
            assert_adagrad_close(gw[k].cpu().numpy(), ref_w[k], ref_g[k], what + f" adagrad core{k} lr={lr} eps={eps}", lr=lr, eps=eps,
                                 state0=state0[k], scale=tol["rtol"] / RTOL)
        # the same backward a second time with per_sample_weights (a weight per lookup in [-0.5, 1.5), a tenth exactly 0), against
        # the weighted float64 reference tests/tt_ref64.py -- the oracle has no weights: a route that drops the weights, or reads them
        # in another order than the lookups', fails here whatever plan it took.  Tolerance: the DEFAULT; a comparison that misses it
        # is looked at again under the rule of tests/test_per_sample_weights_gpu.py -- the fp32 oracle on the one-bag-per-lookup
        # restatement of this case, run only then (it is slow), more than half a default bound from float64 itself: twice its distance,
        # capped at (5e-5, 1e-5).  (Draws from a stream of their own again.)
        rs3 = np.random.RandomState([seed, n, 79])
        psw = (rs3.rand(nnz) * 2.0 - 0.5).astype(np.float32)
        psw[rs3.rand(nnz) < 0.1] = 0.0
        ref64 = R.forward_backward(tables, p, q, r, B, idx, rowidx, tableidx, cores, d_out, per_sample_weights=psw)
        orc = []

        def factor(which, k, ref):
            if tables * nnz * D * 4 > 1 << 30:  # (the restated bag gradients [tables, nnz, D]: too large here -- the default stands)
                return 1.0
            if not orc:
                orc.append(R.oracle_on_restatement(tables, p, q, r, B, idx, rowidx, tableidx, psw, cores, d_out, lr))
            o = orc[0][which]
            f, u = R.widen_factor(o if k is None else o[k], ref)
            print(f"[fuzz] {what} weighted {('out', '', 'grad', 'sgd core')[which]}{'' if k is None else k}: oracle {u:.3f} default bounds from float64 -> bound x{f:.2f}")
            return f

        def close(got, ref, label, which, k):
            try:
                assert_close(got, ref, what + label)
            except AssertionError:
                f = factor(which, k, ref)
                if f <= 1.0:
                    raise
                assert_close(got, ref, what + label, rtol=RTOL * f, atol_scale=ATOL_SCALE * f)

        dpsw = t(psw)
        out = E.tt_forward(1000, tables, B, D, p, q, r, Lt, nnz, t(idx), ri, ti, gc, plan=plan, per_sample_weights=dpsw)
        close(out.cpu().numpy(), ref64["out"], " weighted out", 0, None)
        gw = [t(x) for x in cores]
        E.tt_sgd_backward(1000, D, lr, p, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gw, plan=plan, per_sample_weights=dpsw)
        for k, e in enumerate(R.sgd_step(cores, ref64["grads"], lr)):
            close(gw[k].cpu().numpy(), e, f" weighted sgd core{k} lr={lr}", 3, k)
        e_w, e_s = R.adagrad_step(cores, state0, ref64["grads"], ref64["touched"], lr, eps)
        gw, gs = [t(x) for x in cores], [t(x) for x in state0]
        E.tt_adagrad_backward(1000, D, lr, eps, p, q, r, Lt, nnz, t(idx), ri, ti, t(d_out), gs, gw, plan=plan, per_sample_weights=dpsw)
        for k in range(T):
            def ada(f, k=k):
                R.assert_state_close(gs[k].cpu().numpy(), e_s[k], ref64["grads"][k], what + f" weighted adagrad state{k}", scale=f)
                assert_adagrad_close(gw[k].cpu().numpy(), e_w[k], ref64["grads"][k], what + f" weighted adagrad core{k} lr={lr} eps={eps}",
                                     lr=lr, eps=eps, state0=state0[k], scale=f)

            try:
                ada(1.0)
            except AssertionError:
                f = factor(2, k, ref64["grads"][k])  # (the gradient's factor, as for the state and weights of the per-site file)
                if f <= 1.0:
                    raise
                ada(f)
        route = PR.route_family(PR.route(PR.Geom(tables, p), nnz, int(plan.buf[:8].view(torch.int32)[1]), entry="prologue" if by_prologue else "build",
                                         nb=tables * B))
        routes[route] = routes.get(route, 0) + 1
        n += 1
        E.debug_lds_budget(0)
    return n, routes


def run_cache_cases(seed=0, max_cases=None, budget=None):
    """-> cases run"""
    import tt_embeddings as E

    rs = np.random.RandomState(seed)
    t0, n = time.time(), 0
    while (budget is None or time.time() - t0 < budget) and (max_cases is None or n < max_cases):
        H = int(rs.choice([64, 4096, 1 << 16, 1 << 20]))
        E_ = int(rs.choice([50, 5000, 11_000_000]))
        a = float(rs.choice([1.05, 1.3, 2.0]))
        keys, freq = np.full(H, -1, dtype=np.int64), np.zeros(H, dtype=np.int64)
        for _ in range(int(rs.randint(1, 4))):
            O.update_cache_state((rs.zipf(a, size=int(rs.randint(1, 5000))) % E_).astype(np.int64), keys, freq)
        cs = int(rs.randint(1, 2000))
        state = np.where((keys != -1) & (rs.rand(H) < 0.6), rs.randint(0, cs, size=H), -1).astype(np.int32)
        nnz = int(rs.choice([1, 63, 64, 255, 256, 257, 1000, 4096, 20000, 70000]))
        B = int(rs.choice([1, 5, 64, 512, 3000]))
        B = max(B, nnz // 300)  # (a row hit m times in a bag takes m*g here and g m times in the oracle: keep m modest)
        lens = rs.multinomial(nnz, np.ones(B) / B)
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = (rs.zipf(a, size=nnz) % E_).astype(np.int64)
        exp = O.preprocess_indices(idx, off, 1, False, keys, state)
        got = E.preprocess_indices_sync(t(idx), t(off), 1, False, t(keys), t(state))
        what = f"case {n}: H={H} nnz={nnz} B={B}"
        assert got[3] == exp[3], what + " num_tt"
        ntt = exp[3]
        for k, name in ((0, "colidx"), (1, "rowidx"), (2, "tableidx")):
            assert np.array_equal(got[k].cpu().numpy(), exp[k]), what + " " + name
        if ntt < nnz:
            assert np.array_equal(got[4].cpu().numpy()[ntt:], exp[4][ntt:]), what + " cache locations"
            D = int(rs.choice([4, 64, 60, 128, 7]))
            loc, rowidx = exp[4][ntt:].astype(np.int32), exp[1][ntt:]
            w = rs.randn(cs, D).astype(np.float32)
            out0 = rs.randn(1, B, D).astype(np.float32)
            ref = out0.copy()
            O.cache_forward(B, loc, rowidx, w, ref[0])
            dout = t(out0)
            E.cache_forward(B, nnz - ntt, t(loc), t(rowidx), t(w), dout)
            assert_close(dout.cpu().numpy(), ref, what + f" cache_forward D={D}")
            grad = (rs.rand(B, D) * 0.1).astype(np.float32)
            # reference in float64 (a row can take tens of thousands of adds here: the fp32 oracle's own sequential
            # rounding is then larger than the GPU's, whose partial sums are shorter)
            w_ref = w.astype(np.float64)
            np.subtract.at(w_ref, loc, 0.1 * grad[rowidx].astype(np.float64))
            dw = t(w)
            E.cache_backward_sgd(nnz - ntt, t(grad), t(loc), t(rowidx), 0.1, dw)
            assert_close(dw.cpu().numpy(), w_ref, what + f" cache_backward_sgd D={D}", rtol=5e-5, atol_scale=1e-5)  # (float atomics in hardware order; measured worst: 0.2x the default bound)
            # the weighted backward on the sorted entry over the WHOLE partitioned batch (ttx_cache_weighted_grad_n, then
            # ttx_cache_backward_sorted behind the device-side split point): every cached lookup brings its own row weight x bag
            # gradient.  The bag rows and weights in front of the split point are poisoned -- an extra, in-range gradient row of NaN,
            # NaN weights --: nothing in front of the split point may be read (include/ttx.h).  (Draws from a stream of their own:
            # the cases above stay what they were.)
            rs2 = np.random.RandomState([seed, n, 77])
            psw = (rs2.rand(nnz) * 2 - 0.5).astype(np.float32)
            psw[rs2.rand(nnz) < 0.1] = 0.0
            psw[:ntt] = np.nan
            grad2 = np.concatenate([grad, np.full((1, D), np.nan, dtype=np.float32)])
            row_all = np.concatenate([np.full(ntt, B, dtype=np.int64), rowidx])
            loc_all = t(exp[4].astype(np.int32))
            skip = torch.tensor([ntt], dtype=torch.int32, device=dev)
            scaled = torch.full((nnz, D), float("nan"), device=dev)
            iota = torch.full((nnz,), -1, dtype=torch.int64, device=dev)
            dg2, dpsw, drow = t(grad2), t(psw), t(row_all)
            L = E.lib()
            assert L.ttx_cache_weighted_grad_n(C.c_int64(nnz), C.c_void_p(skip.data_ptr()), C.c_int32(D), C.c_void_p(dg2.data_ptr()),
                                               C.c_void_p(drow.data_ptr()), C.c_void_p(dpsw.data_ptr()), C.c_void_p(scaled.data_ptr()),
                                               C.c_void_p(iota.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            assert torch.equal(iota, torch.arange(nnz, device=dev)), what + " iota must be written for every lookup"
            assert bool(torch.isfinite(scaled[ntt:]).all()) and not bool(scaled[:ntt].any()), what + " scaled rows"
            scaled[:ntt] = float("nan")  # (the sorted entry is owed nothing there either)
            delta = np.zeros((cs, D))
            np.add.at(delta, loc, psw[ntt:].astype(np.float64)[:, None] * grad[rowidx].astype(np.float64))
            # (tests/test_cache_gpu.py::test_sorted_cache_update_edge_cases: a row that takes most of a batch of tens of thousands of
            #  lookups is an fp32 sum of that many terms, here of mixed sign)
            tol = dict(rtol=5e-5, atol_scale=1e-5) if nnz >= 30000 or cs == 1 else {}
            for optim, target in ((E.OPTIM_SGD, t(w)), (E.OPTIM_DENSE, torch.full((cs, D), 7.0, device=dev))):
                E._cache_backward_sorted(optim, nnz, scaled, loc_all, iota, 0.1, 0.0, None, target, skip_dev=skip)
                assert_close(target.cpu().numpy(), w.astype(np.float64) - 0.1 * delta if optim == E.OPTIM_SGD else delta,
                             what + f" weighted sorted cache update optim={optim} D={D}", **tol)
        n += 1
    return n
