"""The photometric loss of gsr_photo_loss_forward / _backward (csrc/photo_loss.hip) restated in numpy, operation for operation
in the order include/gsrast_amd.h states, parametrised by dtype: in float32 it is what the kernels must produce bit for bit
(numpy's float32 +, -, *, / are correctly rounded and never contracted); in float64 it is checked against torch's autograd
of the conv2d composition (tests/test_photo_loss_cpu.py)."""
from __future__ import annotations

import numpy as np

RADIUS = 5
TAPS = 2 * RADIUS + 1


def images(shape, seed):
    """(image, target), float32 [C,H,W] in [0, 1]: noise, the image the target plus a tenth of it clipped (so both ends are
    saturated here and there), and in the four corners, each a quarter of the sides: both black; image == target; the image
    saturated at 1; the target at 0. (On a shape too small for corners the blocks overwrite each other in that order.)"""
    rng = np.random.default_rng(seed)
    C, H, W = shape
    y = rng.random(shape)
    x = np.clip(y + 0.1 * rng.normal(size=shape), 0.0, 1.0)
    h, w = max(1, H // 4), max(1, W // 4)
    x[:, :h, :w] = 0.0
    y[:, :h, :w] = 0.0
    x[:, H - h:, W - w:] = y[:, H - h:, W - w:]
    x[:, :h, W - w:] = 1.0
    y[:, H - h:, :w] = 0.0
    return x.astype(np.float32), y.astype(np.float32)


def window(dtype=np.float32):
    """g[k] = exp(-(k-5)^2 / 4.5) / sum: computed and normalised in double, rounded to `dtype` once."""
    k = np.arange(TAPS, dtype=np.float64) - RADIUS
    g = np.exp(-(k * k) / 4.5)
    return (g / g.sum()).astype(dtype)


def conv(a, g):
    """Zero padded, separable: a horizontal pass, then a vertical one over its result; acc = acc + g[k] * v from acc = 0, k
    ascending (an out-of-image tap contributes g[k] * 0)."""
    C, H, W = a.shape
    dt = a.dtype
    p = np.zeros((C, H, W + 2 * RADIUS), dt)
    p[:, :, RADIUS:RADIUS + W] = a
    h = np.zeros((C, H, W), dt)
    for k in range(TAPS):
        h = h + g[k] * p[:, :, k:k + W]
    p = np.zeros((C, H + 2 * RADIUS, W), dt)
    p[:, RADIUS:RADIUS + H, :] = h
    v = np.zeros((C, H, W), dt)
    for k in range(TAPS):
        v = v + g[k] * p[:, k:k + H, :]
    return v


def maps(x, y, dtype=np.float32):
    """-> dict of the per-pixel maps: m (the SSIM map), d_s11, d_s12, t_mu (what the backward convolves), absdiff."""
    dt = np.dtype(dtype).type
    x, y, g = x.astype(dt), y.astype(dt), window(dt)
    C1, C2, two = dt(0.01 ** 2), dt(0.03 ** 2), dt(2)
    mu1, mu2 = conv(x, g), conv(y, g)
    s11 = conv(x * x, g) - mu1 * mu1
    s22 = conv(y * y, g) - mu2 * mu2
    s12 = conv(x * y, g) - mu1 * mu2
    a1 = two * (mu1 * mu2) + C1
    a2 = two * s12 + C2
    b1 = (mu1 * mu1 + mu2 * mu2) + C1
    b2 = (s11 + s22) + C2
    m = (a1 * a2) / (b1 * b2)
    d_s12 = (two * a1) / (b1 * b2)
    d_s11 = -(m / b2)
    d_mu1 = (two * mu2 * a2) / (b1 * b2) - (two * mu1 * m) / b1
    t_mu = (d_mu1 - two * mu1 * d_s11) - mu2 * d_s12
    return {"m": m, "d_s11": d_s11, "d_s12": d_s12, "t_mu": t_mu, "absdiff": np.abs(x - y)}


def terms(x, y, lam, dtype=np.float32):
    """(loss, l1, ssim) as doubles: the sums of the `dtype` values |x - y| and m taken in float64 (numpy's pairwise order: the
    kernel's order differs, by far less than a float32 ulp). The kernel rounds each of the three to float32 once."""
    q = maps(x, y, dtype)
    n = float(q["m"].size)
    l1 = float(q["absdiff"].astype(np.float64).sum()) / n
    ssim = float(q["m"].astype(np.float64).sum()) / n
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim


def gradient(x, y, lam, up=1.0, dtype=np.float32):
    """dL_dimage = up * (cs * S + cl * sgn); cs = -lam / n and cl = (1 - lam) / n computed in double, rounded once."""
    dt = np.dtype(dtype).type
    x, y, g = x.astype(dt), y.astype(dt), window(dt)
    q = maps(x, y, dtype)
    n = float(x.size)
    cs, cl, two = dt(-lam / n), dt((1.0 - lam) / n), dt(2)
    S = (conv(q["t_mu"], g) + two * x * conv(q["d_s11"], g)) + y * conv(q["d_s12"], g)
    d = x - y
    sgn = (d > 0).astype(dt) - (d < 0).astype(dt)
    return dt(up) * (cs * S + cl * sgn)
