"""helpers shared by the parity tests"""
import numpy as np

# fp32 tolerance of BASELINE.json's north_star: 1e-5 rtol.  atol is tied to the
# magnitude of the reference tensor (sums of a few hundred fp32 products).
RTOL = 1e-5
ATOL_SCALE = 2e-6

LR, EPS = 0.1, 1.0e-4  # tt_embeddings_test.py:268-269


# Every comparison WIDER than the default (rtol 1e-5, atol 2e-6 max|ref|) is recorded with the worst error it actually saw, so
# that DESIGN.md section 5 can carry one table of widened comparisons -- bound next to measurement -- and a regression inside the
# slack is visible (round 4 verdict).  TTX_TOL_REPORT=<file>: the records are written there as JSON lines when the process ends
# (scripts/tolerance_table.py turns them into the table).
_WIDE = {}


def _record_wide(what, rtol, atol_scale, err, ref, atol):
    bound = atol + rtol * np.abs(ref)
    dflt = ATOL_SCALE * atol / max(atol_scale, 1e-300) + RTOL * np.abs(ref)      # what the default tolerance would have allowed
    record_wide_bounds(what, rtol, atol_scale, err, bound, dflt)


def record_wide_bounds(what, rtol, atol_scale, err, bound, dflt):
    """err against an elementwise bound that is wider than `dflt`, the same bound at the default tolerance (the derived bounds of
    assert_adagrad_close(scale=) and tt_ref64.assert_state_close(scale=); rtol, atol_scale: the widened GRADIENT tolerance behind them)"""
    import atexit
    import json
    import os

    path = os.environ.get("TTX_TOL_REPORT")
    if not path:
        return
    test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
    used = float((err / bound).max()) if err.size else 0.0                       # share of the WIDENED bound used (1 = at the limit)
    over = float((err / dflt).max()) if err.size else 0.0                        # worst error in units of the DEFAULT bound
    if not _WIDE:
        def dump():
            with open(path, "a") as f:
                for (t, w), v in _WIDE.items():
                    f.write(json.dumps({"test": t, "what": w, **v}) + "\n")
        atexit.register(dump)
    import re
    key = (test.split("[")[0], re.sub(r"[0-9]+", "#", what)[:80])
    cur = _WIDE.get(key)
    if cur is None or over > cur["worst_over_default"]:
        _WIDE[key] = {"rtol": rtol, "atol_scale": atol_scale, "share_of_bound_used": round(used, 4),
                      "worst_over_default": round(over, 3), "calls": (cur["calls"] + 1 if cur else 1)}
    else:
        cur["calls"] += 1


def assert_close(got, ref, what="", rtol=RTOL, atol_scale=ATOL_SCALE):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} vs {ref.shape}"
    assert np.isfinite(ref).all(), f"{what}: reference has non-finite values"
    assert np.isfinite(got).all(), f"{what}: result has non-finite values"
    atol = atol_scale * max(float(np.abs(ref).max()) if ref.size else 0.0, 1e-30)
    err = np.abs(got - ref)
    if rtol > RTOL or atol_scale > ATOL_SCALE:
        _record_wide(what, rtol, atol_scale, err, ref, atol)
    bad = err > atol + rtol * np.abs(ref)
    if bad.any():
        i = np.unravel_index(np.argmax(err - (atol + rtol * np.abs(ref))), err.shape)
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.size} elements out of tolerance (rtol {rtol}, atol {atol:.3e}); "
            f"worst at {i}: got {got[i]!r} ref {ref[i]!r}")


def sgd_expected(cores, grads, lr=LR):
    """tt_embeddings_test.py:243-246 in fp32"""
    return [c - g * np.float32(lr) for c, g in zip(cores, grads)]


def adagrad_expected(cores, grads, lr=LR, eps=EPS):
    """tt_embeddings_test.py:317-333 in fp32"""
    state = [g * g for g in grads]
    new = [c - (g * np.float32(lr)) / (np.sqrt(s) + np.float32(eps)) for c, g, s in zip(cores, grads, state)]
    return new, state


def assert_adagrad_close(got_w, ref_w, ref_g, what="", lr=LR, eps=EPS, state0=None, scale=1.0):
    """First Adagrad step w - lr*g/(sqrt(s0 + g^2)+eps): its derivative w.r.t. g is
    lr*(eps + s0-terms)/(|g|+eps)^2 <= lr/eps, so a gradient that is within the
    gradient tolerance (RTOL, ATOL_SCALE*max|g|) moves w by up to that factor.
    The gradient itself is checked at the tight tolerance by the dense-mode and
    optimizer-state tests.  state0: the state the step starts from (None: zeros).
    scale: the factor by which the caller's GRADIENT comparison was widened beyond the
    default (tests/test_fused_optimizer_gpu.py: a reference that is itself that far
    from float64); the gradient's share of the bound grows with it."""
    got_w = np.asarray(got_w, dtype=np.float64)
    ref_w = np.asarray(ref_w, dtype=np.float64)
    g = np.abs(np.asarray(ref_g, dtype=np.float64))
    assert np.isfinite(got_w).all() and np.isfinite(ref_w).all(), f"{what}: non-finite values"
    dg = float(scale) * (ATOL_SCALE * max(float(g.max()), 1e-30) + RTOL * g)
    denom = (np.sqrt(g * g + (0.0 if state0 is None else np.asarray(state0, dtype=np.float64))) + eps)
    own = RTOL * np.abs(ref_w) + 2e-7 * max(float(np.abs(ref_w).max()), 1e-30)
    tol = own + lr * dg * (eps + denom) / (denom * denom)
    err = np.abs(got_w - ref_w)
    if scale > 1.0:  # (a widened comparison: into the report like assert_close's)
        record_wide_bounds(what, RTOL * scale, ATOL_SCALE * scale, err, tol, own + lr * (dg / scale) * (eps + denom) / (denom * denom))
    bad = err > tol
    if bad.any():
        i = np.unravel_index(np.argmax(err - tol), err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())}/{bad.size} out of tolerance; worst at {i}: got {got_w[i]!r} "
                             f"ref {ref_w[i]!r} tol {tol[i]:.3e} |g| {g[i]:.3e}")


def rowwise_adagrad_segments_f64(grad, loc, rowidx, lr, eps, state, weight):
    """An INDEPENDENT float64 restatement of the reference's cache_backward_rowwise_adagrad_approx_kernel
    (tt_embeddings_cuda.cu:1735-1795), written from the kernel's own structure -- not from oracle/ttx_oracle.c, which it checks
    (round-5 verdict: the one hot-path kernel whose only pin was the restated oracle).  One "warp" per SEGMENT of equal rowidx
    (cu:1751-1761: a run of cached lookups of one bag): g_avg_square = sum(g^2) / D of the bag's gradient row once per segment
    (cu:1762-1771), then lookup after lookup of the segment (cu:1773-1793): old = state[idx]; state[idx] += g_avg_square;
    multiplier = lr / (sqrt(old + g_avg_square) + eps); weight[idx] -= g * multiplier.  Segments are taken in index order here --
    ONE of the orders the reference's concurrent warps can produce, the only one when no cache row is hit from two segments.
    state [cache_size], weight [cache_size, D]: float64 copies are returned, the inputs are left alone."""
    import numpy as np

    g = np.asarray(grad, dtype=np.float64)
    st, w = np.asarray(state, dtype=np.float64).copy(), np.asarray(weight, dtype=np.float64).copy()
    n, D = len(loc), g.shape[1]
    i = 0
    while i < n:
        row = int(rowidx[i])
        sl = 1
        while i + sl < n and int(rowidx[i + sl]) == row:
            sl += 1
        g_avg_square = float((g[row] * g[row]).sum()) / D
        for k in range(sl):
            idx = int(loc[i + k])
            old = st[idx]
            st[idx] = old + g_avg_square
            w[idx] -= g[row] * (lr * (1.0 / (np.sqrt(old + g_avg_square) + eps)))
        i += sl
    return st, w


# Golden vectors are committed in parts of at most GOLDEN_PART_BYTES each (<name>-<k>.npz, the arrays of <name> spread over them):
# no committed file is larger than 1 MiB.  load_golden() reads them back as one {key: array} mapping.
GOLDEN_PART_BYTES = 1000 * 1024


class GoldenArrays(dict):
    @property
    def files(self):
        return list(self)


def load_golden(path):
    """tests/golden/<name>.npz -> {key: array}, from <name>.npz itself or from its parts <name>-1.npz, <name>-2.npz, ..."""
    import glob
    import os

    stem = path[:-4] if path.endswith(".npz") else path
    parts = [path] if os.path.exists(stem + ".npz") else sorted(glob.glob(glob.escape(stem) + "-*.npz"),
                                                               key=lambda f: int(f[len(stem) + 1:-4]))
    assert parts, f"no golden vectors at {stem}.npz or {stem}-<k>.npz"
    out = GoldenArrays()
    for f in parts:
        with np.load(f) as z:
            out.update((k, z[k]) for k in z.files)
    return out


def save_golden(path, blob):
    """np.savez_compressed of `blob` as parts <name>-1.npz, <name>-2.npz, ... of at most GOLDEN_PART_BYTES each (arrays in
    their insertion order; one part when it all fits); removes the files of an earlier save of <name>"""
    import glob
    import io
    import os

    stem = path[:-4] if path.endswith(".npz") else path
    for f in [stem + ".npz"] + glob.glob(glob.escape(stem) + "-*.npz"):
        if os.path.exists(f):
            os.remove(f)

    def packed(arrays):
        buf = io.BytesIO()
        np.savez_compressed(buf, **arrays)
        return buf.getvalue()

    parts, cur = [], {}
    for k, v in blob.items():
        trial = dict(cur, **{k: v})
        if cur and len(packed(trial)) > GOLDEN_PART_BYTES:
            parts.append(cur)
            cur = {k: v}
        else:
            cur = trial
    parts.append(cur)
    for n, arrays in enumerate(parts, 1):
        data = packed(arrays)
        assert len(data) <= GOLDEN_PART_BYTES, f"{stem}: array(s) {list(arrays)} alone exceed {GOLDEN_PART_BYTES} bytes"
        with open(f"{stem}-{n}.npz", "wb") as f:
            f.write(data)
