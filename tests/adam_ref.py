"""A float64 numpy restatement of ONE torch.optim.Adam / AdamW step (no amsgrad) from a given (w, m, v, step): the reference of
the fused Adam (include/ttx.h "fused Adam", csrc/ttx_adam.hip).  tests/test_adam_cpu.py holds it against torch.optim.Adam and
torch.optim.AdamW in float64; the kernel and module tests then compare against it.

    t = step + 1, bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
    decoupled:  w <- w (1 - lr wd)                     (AdamW)
    g' = g, or g + wd w when wd != 0 and not decoupled (Adam's L2 penalty)
    m <- beta1 m + (1 - beta1) g';  v <- beta2 v + (1 - beta2) g'^2
    w <- w - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
"""
import numpy as np


def f32(x):
    """the value a float hyper-parameter has once it has crossed the C ABI (float arguments), as a Python float"""
    return float(np.float32(x))


def step(w, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
    """-> (w, m, v, step + 1), float64 arrays of w's shape; the inputs are left alone"""
    w, g = np.array(w, dtype=np.float64), np.asarray(g, dtype=np.float64).reshape(np.shape(w))
    m, v = np.array(m, dtype=np.float64).reshape(w.shape), np.array(v, dtype=np.float64).reshape(w.shape)
    b1, b2 = float(betas[0]), float(betas[1])
    lr, eps, wd = float(lr), float(eps), float(weight_decay)
    t = int(step) + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if wd != 0.0:
        if decoupled:
            w = w * (1.0 - lr * wd)
        else:
            g = g + wd * w
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    w = w - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + eps)
    return w, m, v, t


def weight_tolerance(w_ref, m_ref, v_ref, g, dg, step_after, lr, betas, eps, rtol, own_scale=2e-7):
    """The bound on |w - w_ref| when the gradient the step consumed is within `dg` (elementwise) of `g`, the project's rule for
    Adagrad (util.assert_adagrad_close) restated for Adam: dg carried through the update's derivative with respect to g, plus the
    weight's own rounding.  With a = lr / bc1, c = 1 / sqrt(bc2), den = c sqrt(v) + eps (m, v: the reference's NEW moments):
        d(update)/dg = a [(1 - beta1) / den  -  m c (1 - beta2) g / (sqrt(v) den^2)]
    and the bound takes both terms by magnitude."""
    b1, b2 = float(betas[0]), float(betas[1])
    w_ref, m_ref, v_ref = (np.asarray(x, dtype=np.float64) for x in (w_ref, m_ref, v_ref))
    g = np.abs(np.asarray(g, dtype=np.float64)).reshape(w_ref.shape)
    a = float(lr) / (1.0 - b1 ** int(step_after))
    c = 1.0 / np.sqrt(1.0 - b2 ** int(step_after))
    sv = np.sqrt(v_ref)
    den = c * sv + float(eps)
    own = rtol * np.abs(w_ref) + own_scale * max(float(np.abs(w_ref).max()) if w_ref.size else 0.0, 1e-30)
    return own + a * dg * ((1.0 - b1) / den + np.abs(m_ref) * c * (1.0 - b2) * g / (np.maximum(sv, 1e-30) * den * den))


def moment_tolerances(m_ref, v_ref, g, dg, betas, m0):
    """-> (bound on |m - m_ref|, bound on |v - v_ref|): the gradient's bound through m = b1 m0 + (1 - b1) g and
    v = b2 v0 + (1 - b2) g^2 -- (1 - b1) dg and (1 - b2)(2 |g| dg + dg^2) -- plus three fp32 ulps for the products' and the sum's
    rounding: of v itself (its terms are positive), and for m of b1 |m0| + (1 - b1) |g| (m0: the moment the step started from --
    its two terms may cancel, their rounding does not)."""
    b1, b2 = float(betas[0]), float(betas[1])
    m_ref, v_ref = np.asarray(m_ref, dtype=np.float64), np.asarray(v_ref, dtype=np.float64)
    g = np.abs(np.asarray(g, dtype=np.float64)).reshape(m_ref.shape)
    mag = b1 * np.abs(np.asarray(m0, dtype=np.float64)).reshape(m_ref.shape) + (1.0 - b1) * g
    um = 3.0 * np.spacing(mag.astype(np.float32)).astype(np.float64)
    uv = 3.0 * np.spacing(np.abs(v_ref).astype(np.float32)).astype(np.float64)
    return (1.0 - b1) * dg + um, (1.0 - b2) * (2.0 * g * dg + dg * dg) + uv
