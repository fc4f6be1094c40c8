"""The reference of the 3DGS-MCMC calls (gsr_mcmc_noise / _plan / _relocate, include/gsrast_amd_mcmc.h), in numpy.

The noise is float32, operation by operation in the header's order. Standard deviations `s` [N,3], normalised quaternions
`q` [N,4] (real part first), opacities `o` [N] and gates `g` [N] are INPUTS: the GPU tests feed them from
gsrast_amd.autograd.activate, whose bits are those of the kernel's own exp, normalisation and sigmoid by construction, so
that no exponential is compared across implementations (tests/densify_ref.py's rule). The relocation is float64. The plan
and the three relocation steps are written with masks, np.bincount and fancy indexing — not a scan, atomics and a gather.
"""
import math

import numpy as np

from densify_ref import RAW, WIDTHS, build_rotation

F = np.float32
MAX_RATIO = 51
TOP = 1.0 - 2.0 ** -23


def gate_argument(o):
    """t = 100 ((1 - o) - 0.995) in float32: what the gate's sigmoid is applied to."""
    o = np.asarray(o, F)
    return (F(100.0) * ((F(1.0) - o) - F(0.995))).astype(F)


def noise_move(v, s, q, drop=None):
    """Sigma v = R S S R^T v in the dtype of the inputs, in the header's order -> [N,3]. drop=(stage, a, j): one of the
    eighteen products is left out (what a blindness guard feeds) — stage 0: Raj * v[a] of R^T v; stage 1: Raj * w[j] of R w."""
    dt = v.dtype
    R = build_rotation(q.astype(dt))
    s = s.astype(dt)
    first = [[R[:, a, j] * v[:, a] for j in range(3)] for a in range(3)]
    if drop is not None and drop[0] == 0:
        first[drop[1]][drop[2]] = np.zeros_like(v[:, 0])
    u = np.stack([s[:, j] * ((first[0][j] + first[1][j]) + first[2][j]) for j in range(3)], axis=1)
    w = (s * u).astype(dt)
    prod = [[R[:, a, j] * w[:, j] for j in range(3)] for a in range(3)]
    if drop is not None and drop[0] == 1:
        prod[drop[1]][drop[2]] = np.zeros_like(v[:, 0])
    return np.stack([(prod[a][0] + prod[a][1]) + prod[a][2] for a in range(3)], axis=1).astype(dt)


def noise(xyz, noise_in, scaler, s, q, g):
    """gsr_mcmc_noise in float32 -> xyz' [N,3]. g: the gate, activate_opacity(gate_argument(o))."""
    c = (g.astype(F) * F(scaler)).astype(F)
    v = (noise_in.astype(F) * c[:, None]).astype(F)
    return (xyz.astype(F) + noise_move(v, s.astype(F), q.astype(F))).astype(F)


def plan(opacity_logit, logit_min_opacity, o):
    """gsr_mcmc_plan -> (dead_idx i32[dead] ascending, weights f32[N], (dead, alive)). o: the activated opacities."""
    dead = opacity_logit <= F(logit_min_opacity)
    weights = np.where(dead, F(0.0), o.astype(F)).astype(F)
    return np.nonzero(dead)[0].astype(np.int32), weights, (int(dead.sum()), int((~dead).sum()))


def relocated(o, ratio, min_opacity):
    """Step 2 of gsr_mcmc_relocate for one row, in float64, as the header writes it. o: the activated opacity (a float32
    value); min_opacity: the float32 threshold. -> (o_new, D, opacity_logit' as a double, the log-scale shift as a double)"""
    o = float(o)
    with np.errstate(divide="ignore"):
        o_new = -math.expm1(float(np.log1p(np.float64(-o))) / ratio)
    D = 0.0
    for i in range(1, ratio + 1):
        p = 1.0
        for k in range(i):
            p = p * o_new
            term = (float(math.comb(i - 1, k)) * p) / math.sqrt(float(k + 1))
            D = D + term if k % 2 == 0 else D - term
    o_c = min(max(o_new, float(min_opacity)), TOP)
    return o_new, D, math.log(o_c / (1.0 - o_c)), math.log(o / D)


def relocate(raw, moments, sampled, dst, min_opacity, o):
    """gsr_mcmc_relocate. raw: {name: array}, moments: {name: (exp_avg, exp_avg_sq)} for the arrays that have them; sampled,
    dst (or None): int arrays [m]; min_opacity: float32; o: the activated opacities f32[N] (the device's).
    -> dict: raw, moments (new arrays), rejected, counts (c[N]), and want64 {"opacity_logit": f64[N], "shift": f64[N]}:
    the two computed values of the updated rows before their rounding to float32 (NaN elsewhere)."""
    n = raw["xyz"].shape[0]
    P = {k: raw[k].reshape(n, WIDTHS[k]).copy() for k in RAW}
    M = {k: tuple(a.reshape(n, WIDTHS[k]).copy() for a in moments[k]) for k in moments}
    sampled = np.asarray(sampled, np.int64)
    ok = (sampled >= 0) & (sampled < n)
    if dst is not None:
        dst = np.asarray(dst, np.int64)
        ok &= (dst >= 0) & (dst < n)
    # ---- 1. the multiplicities ----
    c = np.bincount(sampled[ok], minlength=n)
    # ---- 2. the sampled rows, once each ----
    hit = np.nonzero(c > 0)[0]
    want_logit, want_shift = np.full(n, np.nan), np.full(n, np.nan)
    for i in hit:
        _, _, want_logit[i], want_shift[i] = relocated(o[i], min(int(c[i]) + 1, MAX_RATIO), F(min_opacity))
    P["opacity_logit"][hit, 0] = want_logit[hit].astype(F)
    P["log_scale"][hit] = (P["log_scale"][hit] + want_shift[hit].astype(F)[:, None]).astype(F)
    for k in M:
        for a in M[k]:
            a[hit] = 0
    # ---- 3. the copies ----
    if dst is not None:
        for k in RAW:
            P[k][dst[ok]] = P[k][sampled[ok]]
            if k in M:
                for a in M[k]:
                    a[dst[ok]] = 0
    shape = lambda k, a: a.reshape(n) if k == "opacity_logit" else a
    return dict(raw={k: shape(k, P[k]) for k in RAW}, moments={k: tuple(shape(k, a) for a in M[k]) for k in M},
                rejected=int((~ok).sum()), counts=c, want64={"opacity_logit": want_logit, "shift": want_shift})


def sample_rows(weights, u):
    """gsrast_amd.mcmc.sample_rows by a linear walk in Python floats (small examples only)."""
    cdf = np.cumsum(np.asarray(weights, np.float64))
    total = cdf[-1]
    out = []
    for x in np.asarray(u, np.float64):
        target = x * total
        rows = [i for i in range(len(cdf)) if cdf[i] > target]
        out.append(rows[0] if rows else max(i for i in range(len(cdf)) if weights[i] > 0))
    return np.asarray(out, np.int64)
