"""References of the opacity compensation (include/gsrast_amd_antialias.h), and the seeded scenes its tests share.

(a) compensation_f32: c and o' = o c in numpy float32, operation for operation as the header words them, for both profiles,
    with the float32 DECISIONS beside them: the cull, the test of d1, the floor, the two clamps and their side. Written from
    the header, not from csrc/antialias.hip.
(b) compensated: the same composition in plain differentiable torch (float64 by default; float32 to measure what that
    arithmetic alone does), in the style of tests/step_autograd_ref.py: the decisions are taken outside, in float32, and
    passed in as masks; torch.autograd differentiates the rest.

BOUNDS: the GPU bound of each gradient array of each seeded scene for the float64 comparison, as a share of the reference
array's largest entry: max(2e-4, 2 e32), e32 = (b) in float32 against itself in float64 on the CPU (same masks). 2e-4 is the
RTOL of the project's backward tests. tests/test_antialias_cpu.py measures e32 and checks the table against it.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

import helpers

F64, F32 = torch.float64, torch.float32
f = np.float32
FLOOR_R = f(0.000025)
MARGIN = 1e-5                  # a float64 decision within this relative distance of its threshold: the row is left out
MAX_LEFT_OUT = 0.02            # ... and at most this share of a scene's rows
FLOOR = 2e-4
ARRAYS = ("means3D", "scales", "rotations")
# ((profile, scene), array) -> bound, for the arrays whose 2 e32 exceeds FLOOR — none does (measured: e32 is at most 2e-6 on
# the conditioned scenes and on the composition frame): every array of every scene is at the floor.
BOUNDS = {}


def bound(scene, array):
    return BOUNDS.get((scene, array), FLOOR)


# ---- (a) float32, operation for operation ---------------------------------------------------------------------------------------
def _mul3(a, b):
    """(A B)[r][c] = (A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c], on [3][3] lists of float32 arrays."""
    return [[(a[r][0] * b[0][c] + a[r][1] * b[1][c]) + a[r][2] * b[2][c] for c in range(3)] for r in range(3)]


def _t(a):
    return [[a[c][r] for c in range(3)] for r in range(3)]


def compensation_f32(means3D, scales, rotations, opacities, view, proj, tan_fovx, tan_fovy, width, height, semantics="gscuda",
                     scale_modifier=1.0):
    """dict of [N] arrays: c, o_out (float32, the header's), and the decisions culled, d1_bad (zero or not finite), floored
    (!(0.000025f < r)), hi_x, lo_x, hi_y, lo_y (bool; the clamps of the rows that are not culled), flows (a gradient goes
    through c)."""
    assert semantics in ("gscuda", "inria")
    m, s, q, o = (np.asarray(a, f) for a in (means3D, scales, rotations, opacities))
    V, Pm = np.asarray(view, f).reshape(16), (np.asarray(proj, f).reshape(16) if proj is not None else None)
    n = m.shape[0]
    k = f(scale_modifier)
    zero = np.zeros(n, f)
    with np.errstate(all="ignore"):
        mx, my, mz, mw = m[:, 0], m[:, 1], m[:, 2], m[:, 3]
        if semantics == "gscuda":
            h = [(Pm[r] * mx + Pm[4 + r] * my) + (Pm[8 + r] * mz + Pm[12 + r] * mw) for r in range(4)]
            iw = f(1.0) / (f(0.001) + h[3])
            px, py, pz = iw * h[0], iw * h[1], iw * h[2]
            culled = (pz < f(0.0)) | (pz > f(1.0)) | (px < f(-1.3)) | (px > f(1.3)) | (py < f(-1.3)) | (py > f(1.3))
            dq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
            inv = f(1.0) / np.sqrt(dq)
            x, y, z, w = q[:, 0] * inv, q[:, 1] * inv, q[:, 2] * inv, q[:, 3] * inv
            D = lambda u: (2.0 * u.astype(np.float64) - 1.0).astype(f)
            E = lambda u: (2.0 * u.astype(np.float64)).astype(f)
            R = [[D(x * x + y * y), E(y * z - x * w), E(y * w + x * z)],
                 [E(y * z + x * w), D(x * x + z * z), E(z * w - x * y)],
                 [E(y * w - x * z), E(z * w + x * y), D(x * x + w * w)]]
            S = [[k * s[:, 0], zero, zero], [zero, k * s[:, 1], zero], [zero, zero, k * s[:, 2]]]
            M = _mul3(R, S)
            Sigma = _mul3(M, _t(M))
            t = [(V[r] * mx + V[4 + r] * my) + (V[8 + r] * mz + V[12 + r] * f(1.0)) for r in range(3)]
            fy = f(height) / (f(2.0) * f(tan_fovy))
            fx = fy
        else:
            t = [((V[r] * mx + V[4 + r] * my) + V[8 + r] * mz) + V[12 + r] for r in range(3)]
            culled = t[2] <= f(0.2)
            r_, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            one, two = f(1.0), f(2.0)
            R = [[one - two * (y * y + z * z), two * (x * y - r_ * z), two * (x * z + r_ * y)],
                 [two * (x * y + r_ * z), one - two * (x * x + z * z), two * (y * z - r_ * x)],
                 [two * (x * z - r_ * y), two * (y * z + r_ * x), one - two * (x * x + y * y)]]
            S = [[k * s[:, 0], zero, zero], [zero, k * s[:, 1], zero], [zero, zero, k * s[:, 2]]]
            M = _mul3(S, _t(R))
            Sigma = _mul3(_t(M), M)
            fx = f(width) / (f(2.0) * f(tan_fovx))
            fy = f(height) / (f(2.0) * f(tan_fovy))
        lx, ly = f(1.3) * f(tan_fovx), f(1.3) * f(tan_fovy)
        gmin = lambda a, b: np.where(b < a, b, a)                # glm::min / max
        gmax = lambda a, b: np.where(a < b, b, a)
        rx, ry, tz = t[0] / t[2], t[1] / t[2], t[2]
        ux, uy = gmin(lx, gmax(-lx, rx)) * tz, gmin(ly, gmax(-ly, ry)) * tz
        J = [[fx / tz, zero, (-fx * ux) / (tz * tz)], [zero, fy / tz, (-fy * uy) / (tz * tz)], [zero, zero, zero]]
        W = [[np.broadcast_to(V[4 * c + r], (n,)) for c in range(3)] for r in range(3)]
        T = _mul3(J, W)
        cv = _mul3(_mul3(T, Sigma), _t(T))
        a0, b, c0 = cv[0][0], cv[1][0], cv[1][1]
        d0 = a0 * c0 - b * b
        ca, cc = a0 + f(0.3), c0 + f(0.3)
        d1 = ca * cc - b * b
        r = d0 / d1
        c = np.sqrt(gmax(FLOOR_R, r))
        d1_bad = (d1 == 0) | ~np.isfinite(d1)
        live = ~culled & ~d1_bad
        c = np.where(live, c, f(1.0)).astype(f)
        o_out = np.where(live, o * c, o).astype(f)
        floored = ~(FLOOR_R < r)
    return {"c": c, "o_out": o_out, "culled": culled, "d1_bad": d1_bad & ~culled, "floored": floored & live, "flows": live & ~floored,
            "hi_x": (lx < rx) & ~culled, "lo_x": (rx < -lx) & ~culled, "hi_y": (ly < ry) & ~culled, "lo_y": (ry < -ly) & ~culled,
            "d1": d1, "r": r}


# ---- (b) differentiable torch ------------------------------------------------------------------------------------------------
def compensated(means3D, scales, rotations, opacities, view, masks, tan_fovx, tan_fovy, width, height, semantics="gscuda",
                scale_modifier=1.0):
    """(o' [N], c [N]) as torch tensors of the inputs' dtype. means3D [N,3], scales [N,3], rotations [N,4], opacities [N]:
    tensors (leaves or graph nodes); view: 16 numbers (a constant: not differentiated). masks: compensation_f32's result —
    `flows` selects the rows whose c is computed here, hi_x / lo_x / hi_y / lo_y fix their clamps, and the other rows take
    the constant masks["c"] (1, or the square root of the floor)."""
    dt = opacities.dtype
    idx = torch.from_numpy(np.nonzero(masks["flows"])[0])
    m, s, q = means3D[idx], scales[idx], rotations[idx]
    inria = semantics == "inria"
    if not inria:
        q = q / torch.sqrt((q * q).sum(1, keepdim=True))
    from step_autograd_ref import _rotation
    R = _rotation(q, semantics)
    M = R * (scale_modifier * s)[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    V = torch.as_tensor(np.asarray(view, np.float32).astype(np.float64).reshape(4, 4).T.copy()).to(dt)      # V[r, c] = view[4 c + r]
    t = m @ V[:3, :3].T + V[:3, 3]
    tz = t[:, 2]
    limx, limy = float(f(1.3) * f(tan_fovx)), float(f(1.3) * f(tan_fovy))
    sel = lambda k: torch.from_numpy(np.asarray(masks[k]))[idx]
    tx = torch.where(sel("hi_x"), limx * tz, torch.where(sel("lo_x"), -limx * tz, t[:, 0]))
    ty = torch.where(sel("hi_y"), limy * tz, torch.where(sel("lo_y"), -limy * tz, t[:, 1]))
    fy = float(f(height) / (f(2.0) * f(tan_fovy)))
    fx = float(f(width) / (f(2.0) * f(tan_fovx))) if inria else fy
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    P = J @ V[:3, :3]
    cov = P @ Sigma @ P.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    d0 = a0 * c0 - b * b
    d1 = (a0 + float(f(0.3))) * (c0 + float(f(0.3))) - b * b
    c_live = torch.sqrt(d0 / d1)
    c = torch.from_numpy(np.asarray(masks["c"], np.float32).astype(np.float64)).to(dt).index_put((idx,), c_live)
    return opacities * c, c


def gradients(scene, cam, g, semantics, scale_modifier=1.0, dtype=F64, masks=None):
    """(b)'s gradients of sum(g * o') by means3D [N,3], scales [N,3], rotations [N,4] and opacities [N] (float64 numpy,
    keyed like ARRAYS plus "opacities"), and its c [N]. scene: dict of float32 arrays (means3D / scales [N,4]); g [N]."""
    masks = masks if masks is not None else masks_of(scene, cam, semantics, scale_modifier)
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).requires_grad_(True)
    m, s, q, o = leaf(scene["means3D"][:, :3]), leaf(scene["scales"][:, :3]), leaf(scene["rotations"]), leaf(scene["opacities"])
    out, c = compensated(m, s, q, o, cam.view, masks, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, semantics, scale_modifier)
    loss = (out * torch.from_numpy(np.asarray(g, np.float32)).to(dtype)).sum()
    got = torch.autograd.grad(loss, [m, s, q, o], allow_unused=True)
    res = {k: (v.detach().to(F64).numpy() if v is not None else np.zeros(tuple(t_.shape)))
           for k, v, t_ in zip(ARRAYS + ("opacities",), got, (m, s, q, o))}
    return res, c.detach().to(F64).numpy()


def masks_of(scene, cam, semantics, scale_modifier=1.0):
    return compensation_f32(scene["means3D"], scene["scales"], scene["rotations"], scene["opacities"], cam.view, cam.proj,
                            cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, semantics, scale_modifier)


def near_a_threshold(scene, cam, semantics, scale_modifier=1.0):
    """(near bool[N], agree bool[N]): rows with a float64 decision within a relative MARGIN of its threshold (the rows left
    out of the float64 comparison), and whether each row's float64 decisions are the float32 ones of compensation_f32."""
    masks = masks_of(scene, cam, semantics, scale_modifier)
    m = scene["means3D"].astype(np.float64)
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    t = m[:, :3] @ V[:3, :3].T + V[:3, 3]
    close = lambda v, thr: np.abs(v - thr) <= MARGIN * abs(thr)
    with np.errstate(all="ignore"):
        if semantics == "gscuda":
            Pm = np.asarray(cam.proj, np.float64).reshape(4, 4).T
            h = m @ Pm.T
            p = h[:, :3] / (float(f(0.001)) + h[:, 3:4])
            lim = float(f(1.3))
            culled = (p[:, 2] < 0) | (p[:, 2] > 1) | (np.abs(p[:, 0]) > lim) | (np.abs(p[:, 1]) > lim)
            near = (np.abs(p[:, 2]) <= MARGIN) | close(p[:, 2], 1.0) | close(np.abs(p[:, 0]), lim) | close(np.abs(p[:, 1]), lim)
        else:
            culled = t[:, 2] <= float(f(0.2))
            near = close(t[:, 2], float(f(0.2)))
        rx, ry = t[:, 0] / t[:, 2], t[:, 1] / t[:, 2]
        lx, ly = float(f(1.3) * f(cam.tan_fovx)), float(f(1.3) * f(cam.tan_fovy))
        near |= ~culled & (close(np.abs(rx), lx) | close(np.abs(ry), ly))
        agree = culled == masks["culled"]
        for k, v in (("hi_x", rx > lx), ("lo_x", rx < -lx), ("hi_y", ry > ly), ("lo_y", ry < -ly)):
            agree &= culled | (v == masks[k])
    # the floor, on r in float64 with the clamps as decided above (through (b) itself, every live row flowing)
    live = ~masks["culled"] & ~masks["d1_bad"]
    all_flow = dict(masks, flows=live)
    with torch.no_grad():
        leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(F64)
        _, c64 = compensated(leaf(scene["means3D"][:, :3]), leaf(scene["scales"][:, :3]), leaf(scene["rotations"]), leaf(scene["opacities"]),
                             cam.view, all_flow, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, semantics, scale_modifier)
    r64 = c64.numpy() ** 2
    with np.errstate(all="ignore"):
        near |= live & close(r64, float(FLOOR_R))
        agree &= ~live | ((~(r64 > float(FLOOR_R))) == masks["floored"]) | ~np.isfinite(r64)
    return near, agree


# ---- the seeded scenes ---------------------------------------------------------------------------------------------------------
W, H = 1200, 911                 # focal 1100 at 45 degrees


@functools.lru_cache(maxsize=None)
def camera(semantics):
    """A rolled camera off the axes. Upstream profile: non-square pixels (focal_x / focal_y = 0.8). Reference profile: the
    tangents handed to the call are 0.75 of the projection's (a frame cropped out of a wider projection), so that rows
    clamped at +-1.3 tan_fov exist that its frustum test (+-1.3 in NDC) does not cull."""
    cam = helpers.posed_camera(W, H, (4.0, -3.0, -6.0), target=(0.1, 0.05, 0.0), roll=0.4, kx=1.25 if semantics == "inria" else 1.0)
    if semantics == "gscuda":
        cam = dataclasses.replace(cam, tan_fovx=float(f(0.75) * f(cam.tan_fovx)), tan_fovy=float(f(0.75) * f(cam.tan_fovy)))
    return cam


def _scene(semantics, n, seed, spread, needles=False, edge_rows=False):
    cam = camera(semantics)
    rng = np.random.default_rng(seed)
    true_tx = cam.tan_fovx / (0.75 if semantics == "gscuda" else 1.0)
    true_ty = cam.tan_fovy / (0.75 if semantics == "gscuda" else 1.0)
    z = np.clip(rng.normal(8.0, 2.0, n), 3.0, 14.0)
    behind = rng.uniform(size=n) < 0.05
    z[behind] = rng.uniform(-3.0, 0.15, behind.sum())
    t = np.stack([rng.uniform(-1.45, 1.45, n) * true_tx * z, rng.uniform(-1.45, 1.45, n) * true_ty * z, z], 1)
    means = np.ones((n, 4), np.float32)
    means[:, :3] = helpers.world_from_view(cam, t)
    log_s = rng.normal(-4.0, 1.0, (n, 1)) + rng.normal(0.0, spread, (n, 3))
    kind = rng.uniform(size=n)
    tiny, large = kind < 0.06, kind > 0.94
    log_s[tiny] = rng.uniform(-9.5, -8.5, (tiny.sum(), 1)) + rng.normal(0.0, 0.1, (tiny.sum(), 3))       # far below a pixel: the floor
    log_s[large] = rng.uniform(-2.0, -1.0, (large.sum(), 1)) + rng.normal(0.0, 0.3, (large.sum(), 3))
    scales = np.full((n, 4), np.e, np.float32)
    scales[:, :3] = np.exp(log_s)
    rot = rng.normal(size=(n, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    if semantics == "gscuda":
        rot *= rng.uniform(0.5, 2.0, (n, 1))                     # its preprocess normalises: non-unit quaternions
    scene = {"means3D": means, "scales": scales, "rotations": rot.astype(np.float32),
             "opacities": rng.uniform(0.05, 0.95, n).astype(np.float32)}
    if edge_rows:
        # scales of 0 and of 1e9 (d1 = 0.09 exactly or not finite), a zero quaternion, a Gaussian in the camera's plane
        rows = rng.choice(np.nonzero(~behind)[0], 12, replace=False)
        scene["scales"][rows[0:3], :3] = 0.0
        scene["scales"][rows[3:6], :3] = 1e9
        scene["scales"][rows[6:8], 0] = 0.0
        scene["rotations"][rows[8:10]] = 0.0
        scene["scales"][rows[10:12], :3] = 3e18                  # squares overflow
    return scene


@functools.lru_cache(maxsize=None)
def conditioned_scene(semantics):
    """4096 Gaussians at depth 8 +- 2, focal 1100, log-scales -4 +- 1 with a per-axis spread of 0.3, and groups far below a
    pixel and far above one: the scene of the float64 comparison (float32 keeps c to e32 ~ 3e-7 here)."""
    return _scene(semantics, 4096, 11 if semantics == "gscuda" else 12, 0.3)


@functools.lru_cache(maxsize=None)
def needle_scene(semantics):
    """Per-axis spread 2.5: needles. float32 loses c itself to the cancellation in a0 c0 - b b here, so the scene serves only
    where float32 is compared with float32 — and carries the rows whose d1 is zero or not finite."""
    return _scene(semantics, 1000, 21 if semantics == "gscuda" else 22, 2.5, edge_rows=True)


def first_rows(scene, n):
    return {k: np.ascontiguousarray(v[:n]) for k, v in scene.items()}


def seed_gradient(n, seed=5):
    """dL/do' [n] float32: random, with exact zeros in a tenth of the rows."""
    rng = np.random.default_rng(seed)
    g = rng.normal(size=n).astype(np.float32)
    g[rng.uniform(size=n) < 0.1] = 0.0
    return g


# ---- the composition frame -------------------------------------------------------------------------------------------------------
CW, CH, CN = 64, 48, 320


def composition_camera():
    return helpers.posed_camera(CW, CH, (2.4, -1.5, -5.0), target=(0.0, 0.0, 0.0), roll=0.4)


@functools.lru_cache(maxsize=None)
def composition_raw(semantics):
    """Raw parameters of a few hundred Gaussians seen from far enough (focal 58) that half of them are compensated by more
    than a tenth; a tenth of them off to the sides or behind the camera. Quaternions at lengths 0.5 .. 2; the upstream
    profile's shs are all sixteen triples, coefficient-major."""
    rng = np.random.default_rng(31 if semantics == "gscuda" else 32)
    xyz = rng.uniform(-1.0, 1.0, (CN, 3)) * (1.3, 1.0, 1.0)
    away = rng.uniform(size=CN) < 0.1
    xyz[away] = rng.uniform(-1.0, 1.0, (away.sum(), 3)) * 2.0 + np.where(rng.uniform(size=(away.sum(), 1)) < 0.5, (9.0, 0.0, 0.0), (3.0, -2.0, -9.0))
    rot = rng.normal(size=(CN, 4))
    rot *= rng.uniform(0.5, 2.0, (CN, 1)) / np.linalg.norm(rot, axis=1, keepdims=True)
    shs = np.zeros((CN, 48))
    shs[:, :3] = rng.uniform(-1.0, 1.0, (CN, 3))
    if semantics == "inria":
        shs = rng.normal(0, 0.35, (CN, 48))
    return {"xyz": xyz.astype(np.float32), "opacity_logit": rng.normal(0.5, 1.5, CN).astype(np.float32),
            "log_scale": (rng.normal(-2.0, 0.7, (CN, 1)) + rng.normal(0.0, 0.3, (CN, 3))).astype(np.float32),
            "rotation": rot.astype(np.float32), "shs": shs.astype(np.float32)}


def composition_scene(semantics):
    """The activated arrays of composition_raw (float32 of tests/activation_ref.py's float64: what the CPU test measures e32
    on; the GPU test takes the device's own activations)."""
    import activation_ref as A
    raw = composition_raw(semantics)
    m, s, q, o = A.activations(raw["xyz"], raw["opacity_logit"], raw["log_scale"], raw["rotation"])
    return {"means3D": m.astype(np.float32), "scales": s.astype(np.float32), "rotations": q.astype(np.float32), "opacities": o.astype(np.float32)}
