"""References for gsr_adam_step / gsrast_amd.optim.GaussianAdam (tests/test_adam_cpu.py, tests/test_gpu_adam.py).

step32  the arithmetic include/gsrast_amd.h defines, in numpy float32 (every numpy float32 operation used here — add,
        subtract, multiply, divide, sqrt — is correctly rounded, as the kernel's are), the six scalars rounded to float32
        once from the double the host computes: what the kernel must give bit for bit.
step64  the textbook formula (Kingma & Ba, algorithm 1, with the eps placement of torch.optim.Adam) in float64: what both
        float32 implementations are judged against.
Both are pure: arrays in, new arrays out. `t` is the optimiser's step count AFTER this step (1 for the first)."""
import math

import numpy as np


def scalars32(lr, beta1, beta2, eps, t):
    """(step_size, rs, b1c, b2, b2c, eps) as float32, each rounded once from its double."""
    return tuple(np.float32(x) for x in (lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t), 1.0 - beta1, beta2,
                                         1.0 - beta2, eps))


def _rows(visible, n):
    if visible is None:
        return np.ones(n, bool)
    visible = np.asarray(visible)
    assert visible.shape == (n,)
    return visible > 0


def step32(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, visible=None):
    """-> (p', m', v'), float32. visible (per row = first axis; None: all): a row with visible <= 0 keeps its p, m and v,
    and its g is not touched (it may be NaN)."""
    p, g, m, v = (np.asarray(a) for a in (p, g, m, v))
    assert all(a.dtype == np.float32 and a.shape == p.shape for a in (p, g, m, v))
    step_size, rs, b1c, b2, b2c, eps32 = scalars32(lr, betas[0], betas[1], eps, t)
    on = _rows(visible, p.shape[0])
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    gg, mm, vv, pp = g[on], m[on], v[on], p[on]
    m_new = mm + b1c * (gg - mm)
    v_new = b2 * vv + b2c * (gg * gg)
    den = np.sqrt(v_new) / rs + eps32
    p_new = pp - step_size * (m_new / den)
    assert all(a.dtype == np.float32 for a in (m_new, v_new, den, p_new))
    p2[on], m2[on], v2[on] = p_new, m_new, v_new
    return p2, m2, v2


def step64(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, visible=None):
    """-> (p', m', v'), float64."""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    beta1, beta2 = betas
    on = _rows(visible, p.shape[0])
    p2, m2, v2 = p.copy(), m.copy(), v.copy()
    m_new = beta1 * m[on] + (1.0 - beta1) * g[on]
    v_new = beta2 * v[on] + (1.0 - beta2) * g[on] * g[on]
    m_hat = m_new / (1.0 - beta1 ** t)
    v_hat = v_new / (1.0 - beta2 ** t)
    p2[on], m2[on], v2[on] = p[on] - lr * m_hat / (np.sqrt(v_hat) + eps), m_new, v_new
    return p2, m2, v2
