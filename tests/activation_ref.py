"""Float64 reference of the activations (gsr_activate_params) and of their backward (gsr_activate_params_backward):
raw values x (opacity logit), s (log-scales), r (unnormalised quaternion, real part first) and the incoming gradients of
the activated arrays -> the gradients of the raw values. tests/test_activations_cpu.py pins the four backward formulas
against central differences of the float64 activations below; the GPU tests compare the kernels with them.
"""
from __future__ import annotations

import numpy as np

F64 = np.float64


def activations(xyz, opacity_logit, log_scale, rotation):
    """(means3D [n,4], scales [n,4], rotations [n,4], opacities [n]) in float64."""
    xyz, x, s, r = (np.asarray(a, F64) for a in (xyz, opacity_logit, log_scale, rotation))
    n = xyz.shape[0]
    means3D = np.concatenate([xyz, np.ones((n, 1))], 1)
    scales = np.concatenate([np.exp(s), np.full((n, 1), np.e)], 1)
    rotations = r / np.sqrt((r * r).sum(1, keepdims=True))
    opacities = 1.0 / (1.0 + np.exp(-x))
    return means3D, scales, rotations, opacities


def backward(opacity_logit, log_scale, rotation, g_means3D, g_scales, g_rotations, g_opacity, radii=None):
    """dL/d(xyz [n,3], opacity_logit [n], log_scale [n,3], rotation [n,4]) in float64 from the gradients of the activated
    arrays: g_means3D / g_scales / g_rotations [n,4] (a fourth column of the first two is ignored: those outputs are
    constants), g_opacity [n]. radii: rows with radii <= 0 are zeros."""
    x, s, r = (np.asarray(a, F64) for a in (opacity_logit, log_scale, rotation))
    gm, gs, gq, go = (np.asarray(a, F64) for a in (g_means3D, g_scales, g_rotations, g_opacity))
    d_xyz = gm[:, :3].copy()
    d_scale = gs[:, :3] * np.exp(s)
    e = np.exp(-np.abs(x))                                  # sigmoid(x) sigmoid(-x) = e / (1 + e)^2, e = exp(-|x|)
    d_op = go * (e / ((1.0 + e) * (1.0 + e)))
    norm = np.sqrt((r * r).sum(1, keepdims=True))
    q = r / norm
    d_rot = (gq - q * (q * gq).sum(1, keepdims=True)) / norm
    if radii is not None:
        off = np.asarray(radii) <= 0
        d_xyz[off], d_scale[off], d_op[off], d_rot[off] = 0.0, 0.0, 0.0, 0.0
    return d_xyz, d_op, d_scale, d_rot


def tolerance(want):
    """The GPU tests' bound per component: 2^-23 of max(|want|, 1e-6 of the Gaussian's largest component of that output) —
    one float rounding of a double result plus one ulp for the difference between two exponentials."""
    want = np.asarray(want, F64)
    rows = np.abs(want).reshape(want.shape[0], -1).max(1).reshape((-1,) + (1,) * (want.ndim - 1))
    return 2.0 ** -23 * np.maximum(np.abs(want), 1e-6 * rows)
