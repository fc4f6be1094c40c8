"""The training step's forward, restated once in plain differentiable torch (float64 by default, CPU, no custom Function):
raw parameters + camera tensors -> color [3,H,W] and depth [H,W]. torch.autograd differentiates the whole composition, so
the gradient it gives owes nothing to oracle/backward_np.py, tests/camera_grad_ref.py, tests/activation_ref.py or to the
way the tests stitch those together: a coupling missing from both the kernels and that stitching shows here.

The semantics are those of oracle/oracle_np.py (profile "gscuda"), oracle/inria_np.py (profile "inria") and
include/gsrast_amd.h (activations: csrc/activation_math.hpp; the depth channel). tests/test_step_autograd_cpu.py pins this
forward to the oracles' images, and measures what float32 arithmetic alone does to its gradients (the table BOUNDS below).
The frames it is used on — scene, camera, cases, loss weights — are tests/step_frames.py's.

Differentiated: the activations; quaternion -> rotation -> cov3D with the modifier; t = V (x, y, z, 1); the clamp of
t.x / t.z, t.y / t.z; J; cov2D = J W Sigma W^T J^T with each profile's focal lengths, the 0.3 dilation and the conic; each
profile's pixel centre; each profile's colour; the blend front to back with the background through the final T; the depth
channel.

Structure (no gradient, passed in as plain arrays so that the CPU oracle's state and the GPU's own state serve alike):
  vis       bool[N]    radii > 0
  ranges    int[T,2], values int[R]   each tile's list in order
  nContrib  int[H,W]   each pixel's last contributor
  clamped   bool[N,3]  the SH colour's clamp flags (upstream profile)
  clx, cly  bool[N], sx, sy float[N]   the float32 clamp decisions on t.x / t.z, t.y / t.z and the side (clamp_decisions_f32)
The decisions inside a pixel (alpha < 1/255, power > 0, the 0.99 clamp, the cut-off) are taken by the restatement itself
in its own arithmetic, without gradient. A pixel on which one of them lies within a relative 1e-5 of its threshold, or
whose last contributor differs from nContrib, is left out of the loss (pixels_to_drop).

forward(..., cut=NAME) detaches exactly one coupling (CUTS): the blindness guards of the tests.

The options of autograd.render beyond colour and depth, all off by default (tests/step_frames.py's FULL_CASES use them;
tests/test_step_full_cpu.py pins them): the 3D smoothing filter between the activations and everything else (filter_3d, a
constant; tests/filter3d_ref.smoothing64), the opacity compensation of antialiased=True formed from this forward's own cov2D
nodes, a feature map of leaf["features"] over a zero background, and the accumulated opacity 1 - T as a map. Their float32
decisions join the structure (with_decisions):
  identity  bool[N]    the smoothing leaves the row as it is (f * f > 0 fails in float32: filter3d_ref.forward_f32)
  flows     bool[N]    c = sqrt(d0 / d1) is computed and differentiated; floored, d1_bad bool[N]: the rows that take a constant
                       instead (the square root of the floor; 1), as antialias_ref.compensation_f32 decides them
No Gaussian is left out for them: rows_near_a_threshold reports the visible rows on which one lies within MARGIN of its
threshold or differs from its float64 twin, and the tests assert that there are none.

The three geometry regularisers, off by default too (tests/step_frames.py's GEOMETRY_CASES; tests/test_step_geometry_cpu.py pins
them): distortion= / distortion_power (the distortion map as the pairwise sum over a pixel's blended records), normals=True
(the per-Gaussian normals of the rotation nodes, composited into a normal map), median= / median_threshold (the values of the
structure's id map). gradients(loss_terms=) adds their loss terms, the normal-consistency term among them (consistency_map,
consistency_pixels: the pixels that carry it). They add to the structure (with_geometry):
  normal_decisions  dict of axis int[N], flipped bool[N], valid bool[N]: normals_ref.gaussian_normals_f32's on the float32 arrays
  median_ids        int[H,W]  the Gaussian each pixel selected, -1 for none (median_ref.forward's, or the device's)
and seven cuts to CUTS."""
from __future__ import annotations

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
CUTS = ("background", "jacobian_mean", "view_direction", "depth_mean", "clamp_to_tz", "modifier", "quat_norm", "cov2D_view",
        # the filter: ds'/ds taken as 1; do'/do taken as 1 (the coefficient not applied to the opacity's gradient); the
        # coefficient's own dependence on the scales dropped
        "filter_scale", "filter_opacity", "filter_coef",
        # the compensation: c a constant; c differentiated along the unsmoothed scales' path (ds'/ds = 1 inside c only)
        "compensation", "compensation_scales",
        # the feature map's geometry (only dL/dF flows); the opacity map
        "feature_geometry", "opacity_map",
        # the distortion map: only the values' path flows; m detached (for "depth": the torch path to xyz and view)
        "distortion_geometry", "distortion_values",
        # the normal map: the per-Gaussian normals detached (only the blend weights flow); the reverse
        "normal_rotation", "normal_weights",
        # the consistency term's depth normal: opacity detached inside depth / opacity; the opacity.detach() factor made
        # differentiable — the WRONG form, kept as modifier_first is, to show that the test tells the two apart
        "depth_normal_opacity", "depth_normal_weight",
        # the median map: its values detached
        "median_values")

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
SH_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435)

_f = lambda x: float(np.float32(x))
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))
ALPHA_MAX = _f(0.99)
MARGIN = 1e-5
FLOOR_R = _f(0.000025)                                       # the floor of d0 / d1 under the compensation's square root ...
C_FLOORED = float(np.sqrt(np.float32(0.000025)))           # ... and a floored row's c: the float32 square root of it

# The GPU bound of gradient array k of a case of tests/step_frames.py, as a share of the reference array's largest entry:
# max(2e-4, 2 e32[k]), e32 = what float32 arithmetic alone does to the array on that frame (this restatement in float32
# against itself in float64, same structure, same dropped pixels). 2e-4 is the RTOL of tests/test_gpu_backward*.py.
# tests/test_step_autograd_cpu.py measures e32 and checks this table against it. Entries: (case, array) -> bound, for the
# arrays whose 2 e32 exceeds the floor — none does (e32 is at most 3.5e-6 on CASES, 5.1e-6 on FULL_CASES and 3.3e-6 on
# GEOMETRY_CASES, which tests/test_step_full_cpu.py and tests/test_step_geometry_cpu.py measure in the same way): every array
# of every case is at the floor.
FLOOR = 2e-4
BOUNDS = {}


def bound(case, array):
    return BOUNDS.get((case, array), FLOOR)


# ---- structure -----------------------------------------------------------------------------------------------------------------
def clamp_decisions_f32(means3D, view, tan_fovx, tan_fovy):
    """(clx, cly, sx, sy): is t.x / t.z (t.y / t.z) beyond +-1.3f tan_fov, and on which side — in float32, in the kernels'
    operation order (as tests/camera_grad_ref.py forms them)."""
    f = np.float32
    v, m, one = np.asarray(view, f).reshape(16), np.asarray(means3D, f), f(1.0)
    with np.errstate(all="ignore"):
        tx = (v[0] * m[:, 0] + v[4] * m[:, 1]) + (v[8] * m[:, 2] + v[12] * one)
        ty = (v[1] * m[:, 0] + v[5] * m[:, 1]) + (v[9] * m[:, 2] + v[13] * one)
        tz = (v[2] * m[:, 0] + v[6] * m[:, 1]) + (v[10] * m[:, 2] + v[14] * one)
        rx, ry = tx / tz, ty / tz
        limx, limy = f(1.3) * f(tan_fovx), f(1.3) * f(tan_fovy)
        cx, cy = np.minimum(limx, np.maximum(-limx, rx)), np.minimum(limy, np.maximum(-limy, ry))
    return rx != cx, ry != cy, np.sign(rx).astype(np.float64), np.sign(ry).astype(np.float64)


def structure_of(means3D, view, tan_fovx, tan_fovy, width, height, radii, ranges, values, n_contrib, clamped=None):
    """The structure dict of forward() from a forward state's arrays (the CPU oracle's, or the GPU's read back)."""
    n = np.asarray(radii).shape[0]
    clx, cly, sx, sy = clamp_decisions_f32(np.asarray(means3D)[:, :3], view, tan_fovx, tan_fovy)

    def u32(a):                                               # (the state's words are unsigned, whatever type carries them)
        a = np.ascontiguousarray(a)
        return (a.view(np.uint32) if a.dtype.itemsize == 4 else a).astype(np.int64)
    return {"vis": np.asarray(radii) > 0,
            "ranges": u32(ranges).reshape(-1, 2),
            "values": u32(values).reshape(-1),
            "nContrib": u32(n_contrib).reshape(height, width),
            "clamped": np.zeros((n, 3), bool) if clamped is None else np.asarray(clamped, bool),
            "clx": clx, "cly": cly, "sx": sx, "sy": sy}


def with_decisions(structure, masks=None, identity=None):
    """structure plus the float32 decisions of the compensation (masks: antialias_ref.compensation_f32's result on the arrays
    the compensation reads) and of the smoothing (identity: filter3d_ref.forward_f32's). The compensation's clamp decisions
    must be the ones the structure already holds for the visible Gaussians: one t, one clamp, read by the conic and by c."""
    out = dict(structure)
    vis = structure["vis"]
    if masks is not None:
        assert not (masks["culled"] & vis).any()
        for a, b in ((masks["hi_x"] | masks["lo_x"], structure["clx"]), (masks["hi_y"] | masks["lo_y"], structure["cly"]),
                     (masks["hi_x"], structure["clx"] & (structure["sx"] > 0)), (masks["hi_y"], structure["cly"] & (structure["sy"] > 0))):
            assert (np.asarray(a)[vis] == np.asarray(b)[vis]).all()
        out.update(flows=np.asarray(masks["flows"], bool), floored=np.asarray(masks["floored"], bool),
                   d1_bad=np.asarray(masks["d1_bad"], bool))
        assert ((out["flows"] ^ out["floored"] ^ out["d1_bad"]) & ~(out["flows"] & out["floored"] & out["d1_bad"]))[vis].all()
    if identity is not None:
        out["identity"] = np.asarray(identity, bool)
    return out


def with_geometry(structure, normal_decisions=None, median_ids=None):
    """structure plus the float32 decisions of the per-Gaussian normals (normals_ref.gaussian_normals_f32's dict on the float32
    arrays the kernel is handed: axis, flipped, valid, each [N]) and the median map's ids (uint32 or int32 [H,W] as
    median_ref.forward or the device gives them; kept as int64 with -1 where nothing was selected)."""
    out = dict(structure)
    if normal_decisions is not None:
        out["normal_decisions"] = {k: np.asarray(normal_decisions[k]) for k in ("axis", "flipped", "valid")}
    if median_ids is not None:
        ids = np.ascontiguousarray(median_ids)
        ids = (ids.view(np.uint32) if ids.dtype.itemsize == 4 else ids).astype(np.int64)
        out["median_ids"] = np.where(ids >= structure["vis"].shape[0], -1, ids)
    return out


# ---- the differentiable forward ----------------------------------------------------------------------------------------------
def leaves(raw, cam, dtype=F64, colors=False, features=None, constant=(), distortion_values=None, median_values=None):
    """The leaf tensors forward() is differentiated by: the raw parameters (and `colors` for the colors_precomp case,
    `features` [N,C] for the feature map, distortion_values / median_values [N] for a distortion= / median= tensor) and the
    three camera tensors, from their float32 values. constant: names of the camera tensors that are no leaves (the view
    matrix under antialiased=True or normals=True)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dtype).requires_grad_(True)
    out = {k: t(raw[k]) for k in RAW}
    if colors:
        out["colors"] = t(raw["colors"])
    if features is not None:
        out["features"] = t(features)
    if distortion_values is not None:
        out["distortion_values"] = t(distortion_values)
    if median_values is not None:
        out["median_values"] = t(median_values)
    out.update(view=t(cam.view), proj=t(cam.proj), cam_pos=t(cam.cam_pos))
    for k in constant:
        out[k] = out[k].detach()
    return out


def _sh_colour(deg, d, sh):
    """0.5 + sum_k B_k(d) sh[k]: d [n,3] unit directions, sh [n,16,3]."""
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    res = SH_C0 * sh[:, 0]
    if deg > 0:
        res = res - SH_C1 * y * sh[:, 1] + SH_C1 * z * sh[:, 2] - SH_C1 * x * sh[:, 3]
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + SH_C2[0] * xy * sh[:, 4] + SH_C2[1] * yz * sh[:, 5] + SH_C2[2] * (2.0 * zz - xx - yy) * sh[:, 6]
               + SH_C2[3] * xz * sh[:, 7] + SH_C2[4] * (xx - yy) * sh[:, 8])
    if deg > 2:
        res = (res + SH_C3[0] * y * (3.0 * xx - yy) * sh[:, 9] + SH_C3[1] * xy * z * sh[:, 10]
               + SH_C3[2] * y * (4.0 * zz - xx - yy) * sh[:, 11] + SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy) * sh[:, 12]
               + SH_C3[4] * x * (4.0 * zz - xx - yy) * sh[:, 13] + SH_C3[5] * z * (xx - yy) * sh[:, 14]
               + SH_C3[6] * x * (xx - 3.0 * yy) * sh[:, 15])
    return res + 0.5


def _rotation(q, profile):
    """[n,3,3] (math rows / columns). gscuda: of (x, y, z, w) = q, which its preprocess has normalised; upstream: of the raw
    (r, x, y, z) = q."""
    if profile == "gscuda":
        x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        rows = [[2.0 * (x * x + y * y) - 1.0, 2.0 * (y * z - x * w), 2.0 * (y * w + x * z)],
                [2.0 * (y * z + x * w), 2.0 * (x * x + z * z) - 1.0, 2.0 * (z * w - x * y)],
                [2.0 * (y * w - x * z), 2.0 * (z * w + x * y), 2.0 * (x * x + w * w) - 1.0]]
    else:
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        rows = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y)],
                [2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x)],
                [2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y)]]
    return torch.stack([torch.stack(row, 1) for row in rows], 1)


def forward(leaf, structure, tan_fovx, tan_fovy, width, height, *, background, profile="gscuda", sh_degree=0,
            scale_modifier=1.0, depth=False, cut=None, filter_3d=None, antialiased=False, opacity=False, modifier_first=False,
            distortion=None, distortion_power=2, normals=False, median=None, median_threshold=0.5):
    """(color [3,H,W], depth [H,W] or None, aux). leaf: dict of tensors xyz [N,3], opacity_logit [N], log_scale [N,3],
    rotation [N,4], shs [N,48], view [16], proj [16], cam_pos [3] and optionally colors [N,3] (composited as given, no SH).
    aux: the activated tensors means3D [N,3], scales [N,3], rotations [N,4], opacities [N] (graph nodes: differentiate by them
    for the gradients gsr_backward returns), finalT [H,W], last [H,W] (this forward's last contributor) and near [H,W]
    (a decision of the pixel within MARGIN of its threshold), visible (the indices of the visible Gaussians), per_gaussian
    (graph nodes over the visible Gaussians: mean2D [n,2], cov2D [n,3] = (a, b, c) dilated, colors [n,3], depths [n] or None —
    what the blend reads, for the per-Gaussian sums of the render backward) and cov3D [n,6].

    filter_3d [N] (float32 values, a constant): the activated (scales, opacities) become filter3d_ref.smoothing64's, and
    everything downstream reads those — the modifier multiplies the SMOOTHED scale. aux["scales"] / ["opacities"] stay the
    activated nodes; the smoothed ones are aux["scales_smoothed"] / ["opacities_smoothed"]. modifier_first=True is the WRONG
    order (the smoothing of the modified scale), kept for the test that shows the image tells the two apart.
    antialiased: the blend's opacity is o c, c = sqrt(max(0.000025, d0 / d1)) with d0 the determinant of this forward's cov
    before the dilation and d1 the one after it — the nodes the conic is made of. aux["compensation"] [n]; per_gaussian
    gains "opacities" [n], the opacity the blend reads.
    leaf["features"] [N,C]: aux["feature_map"] [C,H,W] = sum F_i alpha_i T_i over a zero background. opacity=True:
    aux["opacity_map"] [H,W] = 1 - T. Both are graph nodes. aux["rows"]: float64 numpy over the visible Gaussians of what
    the row decisions are taken on (rx, ry = t.x / t.z, t.y / t.z; r = d0 / d1 and d1 when antialiased). aux["blended"]
    bool[n]: some pixel composites the Gaussian.

    distortion: "depth" or "values" (leaf["distortion_values"] [N]); aux["distortion_map"] [H,W] is the header's definition
    (include/gsrast_amd_distortion.h) written as the pairwise sum over the records each pixel blends, with w = alpha T of this
    forward: power 2, sum_i sum_j w_i w_j (m_i - m_j)^2; power 1, the signed form in list order, 2 sum_i w_i sum_{j<i} w_j
    (m_i - m_j). No moment recurrence. "depth": m = row 2 of the view matrix times (x, y, z, 1), from the xyz and view leaves.
    normals=True: the per-Gaussian normals are normals_ref.gaussian_normals64 of this forward's rotation nodes under
    structure["normal_decisions"] (the view matrix a constant there), composited like features over a zero background into
    aux["normal_map"] [3,H,W]; aux["rows"] gains what their decisions are taken on (rows_near_a_threshold).
    median: "depth" or "values" (leaf["median_values"]); aux["median_map"] [H,W] = values[structure["median_ids"]], 0 where
    the id is -1. The selection is recomputed here without gradient — the last blended record with the transmittance in front
    of it above float32(median_threshold) — as aux["median_selected"] (global ids, -1: none); aux["median_differs"] [H,W]
    is where it is not the structure's (pixels_to_drop adds those), and a pixel with a blended record whose T lies within
    MARGIN of the threshold joins `near`."""
    assert cut is None or cut in CUTS, cut
    assert distortion in (None, "depth", "values") and median in (None, "depth", "values") and distortion_power in (1, 2)
    assert distortion is not None or cut not in ("distortion_geometry", "distortion_values")
    assert normals or cut not in ("normal_rotation", "normal_weights")
    assert median is not None or cut != "median_values"
    assert filter_3d is not None or (not modifier_first and cut not in ("filter_scale", "filter_opacity", "filter_coef"))
    assert cut != "compensation_scales" or (antialiased and filter_3d is not None)
    assert cut != "compensation" or antialiased
    assert profile in ("gscuda", "inria") and depth in (False, True, "inverse")
    inria = profile == "inria"
    dt = leaf["xyz"].dtype
    cst = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dt)
    # -- the activations
    means3D = leaf["xyz"] * 1.0
    scales = torch.exp(leaf["log_scale"])
    norm = torch.sqrt((leaf["rotation"] * leaf["rotation"]).sum(1, keepdim=True))
    rotations = leaf["rotation"] / (norm.detach() if cut == "quat_norm" else norm)
    opacities = 1.0 / (1.0 + torch.exp(-leaf["opacity_logit"]))
    aux = {"means3D": means3D, "scales": scales, "rotations": rotations, "opacities": opacities}
    idx = torch.from_numpy(np.nonzero(structure["vis"])[0])
    n = idx.numel()
    s_all, o_all = scales, opacities
    if filter_3d is not None:
        from filter3d_ref import smoothing64
        ident = torch.from_numpy(np.asarray(structure["identity"], bool))
        s_in = scale_modifier * scales if modifier_first else scales
        s_all, o_all = smoothing64(s_in, opacities, cst(np.asarray(filter_3d, np.float32)), ident)
        if cut == "filter_scale":
            s_all = s_in + (s_all - s_in).detach()
        elif cut in ("filter_opacity", "filter_coef"):
            coef = torch.where(ident, torch.ones_like(opacities), o_all / opacities)
            o_all = (opacities.detach() * coef + (opacities - opacities.detach()) if cut == "filter_opacity"
                     else opacities * coef.detach())
        aux.update(scales_smoothed=s_all, opacities_smoothed=o_all)
    m, s, q, o = means3D[idx], s_all[idx], rotations[idx], o_all[idx]
    # -- cov3D = R diag(mod s)^2 R^T
    if not inria:
        qn = torch.sqrt((q * q).sum(1, keepdim=True))
        q = q / (qn.detach() if cut == "quat_norm" else qn)
    R = _rotation(q, profile)
    if modifier_first:
        ms = s
    else:
        ms = s + (s * (scale_modifier - 1.0)).detach() if cut == "modifier" else scale_modifier * s
    M = R * ms[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    # -- t = V (x, y, z, 1)
    V = leaf["view"].reshape(4, 4).T                         # V[r, c] = view[4 c + r]
    t = m @ V[:3, :3].T + V[:3, 3]
    tj = t.detach() if cut == "jacobian_mean" else t
    tz = tj[:, 2]
    limx, limy = float(np.float32(1.3) * np.float32(tan_fovx)), float(np.float32(1.3) * np.float32(tan_fovy))
    clx, cly = (torch.from_numpy(structure[k])[idx] for k in ("clx", "cly"))
    sx, sy = (cst(structure[k])[idx] for k in ("sx", "sy"))
    tz_c = tz.detach() if cut == "clamp_to_tz" else tz
    tx = torch.where(clx, sx * limx * tz_c, tj[:, 0])
    ty = torch.where(cly, sy * limy * tz_c, tj[:, 1])
    fy = float(np.float32(height) / (np.float32(2.0) * np.float32(tan_fovy)))
    fx = float(np.float32(width) / (np.float32(2.0) * np.float32(tan_fovx))) if inria else fy
    zero = torch.zeros_like(tz)
    J = torch.stack([torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -(fy * ty) / (tz * tz)], 1)], 1)
    Wm = V[:3, :3].detach() if cut == "cov2D_view" else V[:3, :3]
    P = J @ Wm
    cov = P @ Sigma @ P.transpose(1, 2)
    cov2D = torch.stack([cov[:, 0, 0] + _f(0.3), cov[:, 0, 1], cov[:, 1, 1] + _f(0.3)], 1)
    ca, cb, cc = cov2D[:, 0], cov2D[:, 1], cov2D[:, 2]
    det = ca * cc - cb * cb
    A, B, C = cc / det, -cb / det, ca / det
    rows = {"rx": (t[:, 0] / t[:, 2]).detach().to(F64).numpy(), "ry": (t[:, 1] / t[:, 2]).detach().to(F64).numpy()}
    # -- the compensation of the 0.3 dilation, from the nodes above
    comp = None
    if antialiased:
        cv, d1 = cov, det
        if cut == "compensation_scales":                       # (the same values along another path: ds'/ds = 1 inside c)
            s_c = scales[idx] + (s - scales[idx]).detach()
            Mc = R * (scale_modifier * s_c)[:, None, :]
            cv = P @ (Mc @ Mc.transpose(1, 2)) @ P.transpose(1, 2)
            d1 = (cv[:, 0, 0] + _f(0.3)) * (cv[:, 1, 1] + _f(0.3)) - cv[:, 0, 1] * cv[:, 0, 1]
        ratio = (cv[:, 0, 0] * cv[:, 1, 1] - cv[:, 0, 1] * cv[:, 0, 1]) / d1
        flows = torch.from_numpy(structure["flows"])[idx]
        const = torch.where(torch.from_numpy(structure["floored"])[idx], torch.full_like(ratio, C_FLOORED), torch.ones_like(ratio))
        comp = torch.where(flows, torch.sqrt(torch.where(flows, ratio, torch.ones_like(ratio))), const.detach())
        if cut == "compensation":
            comp = comp.detach()
        o = o * comp
        rows.update(r=ratio.detach().to(F64).numpy(), d1=d1.detach().to(F64).numpy())
    # -- the pixel centre
    Pm = leaf["proj"].reshape(4, 4).T
    h = m @ Pm[:, :3].T + Pm[:, 3]                            # (the activated mean's w is 1 under either profile)
    if inria:
        pw = 1.0 / (h[:, 3] + _f(0.0000001))
        mx, my = ((h[:, 0] * pw + 1.0) * width - 1.0) * 0.5, ((h[:, 1] * pw + 1.0) * height - 1.0) * 0.5
    else:
        pw = 1.0 / (_f(0.001) + h[:, 3])
        mx, my = (h[:, 0] * pw * 0.5 + 0.5) * width, (h[:, 1] * pw * 0.5 + 0.5) * height
    mean2D = torch.stack([mx, my], 1)
    mx, my = mean2D[:, 0], mean2D[:, 1]
    # -- the colour
    if "colors" in leaf:
        rgb = leaf["colors"][idx]
    elif inria:
        dv = m - leaf["cam_pos"][None, :]
        if cut == "view_direction":
            dv = dv.detach()
        d = dv / torch.sqrt((dv * dv).sum(1, keepdim=True))
        raw_rgb = _sh_colour(min(3, max(0, int(sh_degree))), d, leaf["shs"][idx].reshape(n, 16, 3))
        rgb = torch.where(torch.from_numpy(structure["clamped"])[idx], torch.zeros_like(raw_rgb), raw_rgb)
    else:
        rgb = 0.5 + 0.4 * leaf["shs"][idx][:, :3]
    rgb = rgb * 1.0
    # -- the depth values
    dval = None
    if depth:
        dval = 1.0 / t[:, 2] if depth == "inverse" else t[:, 2]
        if cut == "depth_mean":
            dval = dval.detach()
        dval = dval * 1.0
    # -- the values of the distortion and median maps; the per-Gaussian normals
    z_all = means3D @ V[2, :3] + V[2, 3]                         # (its own nodes: the torch path of "depth" beside the rasterizer's t)
    dist_m = med_m = nrm = None
    if distortion is not None:
        dist_m = (z_all if distortion == "depth" else leaf["distortion_values"] * 1.0)[idx]
        if cut == "distortion_values":
            dist_m = dist_m.detach()
    if median is not None:
        med_m = z_all if median == "depth" else leaf["median_values"] * 1.0
        if cut == "median_values":
            med_m = med_m.detach()
        thr = float(np.float32(median_threshold))
    if normals:
        from normals_ref import gaussian_normals64
        dec = {k: np.asarray(v)[idx.numpy()] for k, v in structure["normal_decisions"].items()}
        nrm = gaussian_normals64(rotations[idx], leaf["view"].detach(), dec, profile)
        if cut == "normal_rotation":
            nrm = nrm.detach()
        with torch.no_grad():                                     # what the normals' decisions are taken on, in this arithmetic
            nw = R[torch.arange(n), :, torch.from_numpy(np.asarray(dec["axis"], np.int64))]
            nv = nw @ V[:3, :3].T
            rows.update(normal_dot=(nv * t).sum(1).to(F64).numpy(), normal_length=torch.sqrt((nv * nv).sum(1)).to(F64).numpy(),
                        t_length=torch.sqrt((t * t).sum(1)).to(F64).numpy(), normal_scales=s.detach().to(F64).numpy())
    # -- the blend, tile by tile: [records, pixels]
    local = np.full(structure["vis"].shape[0], -1, np.int64)
    local[idx.numpy()] = np.arange(n)
    gx, gy = (width + 15) // 16, (height + 15) // 16
    cutoff = _f(1e-4) if inria else _f(0.001)
    bg = cst(background)
    color = torch.zeros((3, height, width), dtype=dt)
    dmap = torch.zeros((height, width), dtype=dt) if depth else None
    feat = leaf["features"][idx] if "features" in leaf else None
    fmap = torch.zeros((feat.shape[1], height, width), dtype=dt) if feat is not None else None
    omap = torch.zeros((height, width), dtype=dt) if opacity else None
    dist = torch.zeros((height, width), dtype=dt) if dist_m is not None else None
    nmap = torch.zeros((3, height, width), dtype=dt) if normals else None
    msel = torch.full((height, width), -1, dtype=torch.int64) if median is not None else None
    finalT = torch.ones((height, width), dtype=dt)
    last = torch.zeros((height, width), dtype=torch.int64)
    near = torch.zeros((height, width), dtype=torch.bool)
    blended = torch.zeros(n, dtype=torch.bool)
    for tyi in range(gy):
        for txi in range(gx):
            r0, r1 = (int(v) for v in structure["ranges"][tyi * gx + txi])
            ya, yb, xa, xb = tyi * 16, min(height, tyi * 16 + 16), txi * 16, min(width, txi * 16 + 16)
            ids = torch.from_numpy(local[structure["values"][r0:r1]]) if r1 > r0 else torch.zeros(0, dtype=torch.int64)
            assert (ids >= 0).all()
            py, px = torch.meshgrid(torch.arange(ya, yb), torch.arange(xa, xb), indexing="ij")
            px, py = px.reshape(-1).to(dt), py.reshape(-1).to(dt)
            L, npx = ids.numel(), px.numel()
            dx, dy = mx[ids][:, None] - px[None, :], my[ids][:, None] - py[None, :]
            power = -0.5 * (A[ids][:, None] * dx * dx + C[ids][:, None] * dy * dy) - B[ids][:, None] * dx * dy
            a_raw = o[ids][:, None] * torch.exp(power)
            alpha = torch.clamp(a_raw, max=ALPHA_MAX)
            with torch.no_grad():
                skip = (power > 0) | (alpha < ALPHA_MIN)
                a0 = torch.where(skip, torch.zeros_like(alpha), alpha)
                T0 = torch.cat([torch.ones((1, npx), dtype=dt), torch.cumprod(1.0 - a0, 0)[:-1]], 0) if L else a0
                test = T0 * (1.0 - a0)
                stop = ~skip & (test < cutoff)
                order = torch.arange(L)[:, None].expand(L, npx)
                none = torch.zeros(npx, dtype=torch.int64)
                first = torch.where(stop, order, torch.full_like(order, L)).min(0).values if L else none
                dead = order >= first[None, :]
                on = ~skip & ~dead                                        # the records the pixel composites
                seen = order <= first[None, :]                            # the records whose decisions the pixel takes
                close = lambda v, thr: (v - thr).abs() <= MARGIN * thr
                nr = seen & ((power.abs() <= MARGIN) | close(a_raw, ALPHA_MIN)
                             | (~skip & (close(a_raw, ALPHA_MAX) | close(test, cutoff))))
                lst = torch.where(on, order + 1, torch.zeros_like(order)).max(0).values if L else none
            if L:
                blended[ids] |= on.any(1)
            a = torch.where(on, alpha, torch.zeros_like(alpha))
            Tx = torch.cat([torch.ones((1, npx), dtype=dt), torch.cumprod(1.0 - a, 0)[:-1]], 0) if L else a
            wgt = a * Tx
            Tf = torch.prod(1.0 - a, 0) if L else torch.ones(npx, dtype=dt)
            Tb = Tf.detach() if cut == "background" else Tf
            shape = (yb - ya, xb - xa)
            color[:, ya:yb, xa:xb] = ((wgt.T @ rgb[ids]).T + bg[:, None] * Tb[None, :]).reshape(3, *shape)
            if depth:
                dmap[ya:yb, xa:xb] = (wgt * dval[ids][:, None]).sum(0).reshape(shape)
            if feat is not None:
                wgt_f = wgt.detach() if cut == "feature_geometry" else wgt
                fmap[:, ya:yb, xa:xb] = (wgt_f.T @ feat[ids]).T.reshape(-1, *shape)
            if dist_m is not None and L:
                mv = dist_m[ids]
                diff = mv[:, None] - mv[None, :]                              # [i, j]: m_i - m_j
                pair = diff * diff if distortion_power == 2 else 2.0 * torch.tril(diff, -1)      # (power 1: the records j < i in front)
                wgt_d = wgt.detach() if cut == "distortion_geometry" else wgt
                dist[ya:yb, xa:xb] = ((pair @ wgt_d) * wgt_d).sum(0).reshape(shape)
            if normals:
                wgt_n = wgt.detach() if cut == "normal_weights" else wgt
                nmap[:, ya:yb, xa:xb] = (wgt_n.T @ nrm[ids]).T.reshape(3, *shape)
            if median is not None and L:
                with torch.no_grad():
                    Tb4 = Tx.detach()
                    at = torch.where(on & (Tb4 > thr), order + 1, torch.zeros_like(order)).max(0).values
                    gl = torch.from_numpy(np.asarray(structure["values"][r0:r1], np.int64))
                    msel[ya:yb, xa:xb] = torch.where(at > 0, gl[(at - 1).clamp_min(0)], torch.full_like(at, -1)).reshape(shape)
                    nr = nr | (on & ((Tb4 - thr).abs() <= MARGIN * thr))
            if opacity:
                omap[ya:yb, xa:xb] = (1.0 - (Tf.detach() if cut == "opacity_map" else Tf)).reshape(shape)
            finalT[ya:yb, xa:xb] = Tf.detach().reshape(shape)
            last[ya:yb, xa:xb] = lst.reshape(shape)
            near[ya:yb, xa:xb] = (nr.any(0) if L else torch.zeros(npx, dtype=torch.bool)).reshape(shape)
    aux.update(finalT=finalT.numpy(), last=last.numpy(), near=near.numpy(), visible=idx.numpy(),
               per_gaussian={"mean2D": mean2D, "cov2D": cov2D, "colors": rgb, "depths": dval},
               feature_map=fmap, opacity_map=omap, compensation=comp, rows=rows, blended=blended.numpy(),
               cov3D=torch.stack([Sigma[:, 0, 0], Sigma[:, 0, 1], Sigma[:, 0, 2], Sigma[:, 1, 1], Sigma[:, 1, 2],
                                  Sigma[:, 2, 2]], 1).detach())
    if antialiased:
        aux["per_gaussian"]["opacities"] = o
    if dist_m is not None:
        aux["distortion_map"] = dist
    if normals:
        aux["normal_map"] = nmap
    if median is not None:
        mid = torch.from_numpy(np.asarray(structure["median_ids"], np.int64))
        aux.update(median_map=torch.where(mid >= 0, med_m[mid.clamp_min(0)], torch.zeros((), dtype=dt)),
                   median_selected=msel.numpy(), median_differs=msel.numpy() != structure["median_ids"])
    return color, dmap, aux


def rows_near_a_threshold(aux, structure, tan_fovx, tan_fovy, filter_3d=None, antialiased=False, normals=False):
    """(near, differ): bool over aux["visible"] — a row decision of the compensation or of the smoothing within a relative
    MARGIN of its threshold in float64, or taken otherwise in float64 than the float32 decision in `structure`. The
    decisions: the two clamps, and with antialiased r = d0 / d1 against the floor and d1 (zero or not finite); with
    filter_3d, f * f > 0; with normals, the per-Gaussian normal's: the two smallest (smoothed) scales within a relative MARGIN
    of each other or another shortest axis in float64, the flip's dot product nv . t within MARGIN of 0 relative to |nv| |t| or of
    another sign, and the normal's length against 0. aux: of the uncut float64 forward()."""
    vis, rows = aux["visible"], aux["rows"]
    near, differ = np.zeros(vis.size, bool), np.zeros(vis.size, bool)
    close = lambda v, thr: np.abs(v - thr) <= MARGIN * thr
    for k, mask, tan in (("rx", "clx", tan_fovx), ("ry", "cly", tan_fovy)):
        lim = float(np.float32(1.3) * np.float32(tan))
        near |= close(np.abs(rows[k]), lim)
        differ |= (np.abs(rows[k]) > lim) != structure[mask][vis]
    if antialiased:
        bad = ~np.isfinite(rows["d1"]) | (rows["d1"] == 0)
        near |= ~bad & (close(rows["r"], FLOOR_R) | (np.abs(rows["d1"]) <= MARGIN))
        differ |= (bad != structure["d1_bad"][vis]) | (~bad & (~(rows["r"] > FLOOR_R) != structure["floored"][vis]))
    if filter_3d is not None:
        f = np.asarray(filter_3d, np.float32).astype(np.float64)[vis]
        differ |= ~(f * f > 0.0) != structure["identity"][vis]
        near |= (f != 0) & (f * f <= float(np.finfo(np.float32).tiny) * (1.0 + MARGIN))
    if normals:
        dec = {k: np.asarray(v)[vis] for k, v in structure["normal_decisions"].items()}
        sc = rows["normal_scales"]
        two = np.sort(sc, 1)[:, :2]
        near |= (two[:, 1] - two[:, 0]) <= MARGIN * two[:, 1]
        axis = np.zeros(vis.size, np.int64)                       # (the header's rule: the first of equal scales)
        for k in (1, 2):
            axis = np.where(sc[:, k] < sc[np.arange(vis.size), axis], k, axis)
        length = rows["normal_length"]
        near |= (np.abs(rows["normal_dot"]) <= MARGIN * length * rows["t_length"]) | (length <= MARGIN)
        differ |= (axis != dec["axis"]) | ((rows["normal_dot"] > 0) != dec["flipped"]) | ((length > 0) != dec["valid"])
    return near, differ


def pixels_to_drop(aux, structure):
    """bool[H,W]: the pixels left out of the loss — a float64 decision within a relative 1e-5 of its threshold, or a last
    contributor that differs from the forward state's nContrib, or (median=) a selected record that is not the structure's.
    aux: of the uncut float64 forward()."""
    drop = aux["near"] | (aux["last"] != structure["nContrib"])
    return drop | aux["median_differs"] if "median_differs" in aux else drop


def eroded(keep):
    """keep without the pixels any of whose four neighbours is not kept."""
    out = keep.copy()
    out[1:] &= keep[:-1]
    out[:-1] &= keep[1:]
    out[:, 1:] &= keep[:, :-1]
    out[:, :-1] &= keep[:, 1:]
    return out


def depth_normal_pixels(surface, tan_fov, semantics, decisions):
    """(near, differ) bool[H,W] of the depth normal of the float64 image `surface` against the float32 decisions
    (normals_ref.depth_normals_f32's dict on the float32 image): near — where the four neighbours are usable, the flip's dot
    product c . r within MARGIN of 0 relative to |c| |r|, or the cross product's length |c| within MARGIN of 0 relative to
    |dv| |dh| (the two differences it is the product of); differ — the neighbours' usability (finite and > 0), the flip or
    the validity taken otherwise in float64."""
    from normals_ref import ndc
    D = np.asarray(surface, np.float64)
    H, W = D.shape
    near, differ = np.zeros((H, W), bool), np.zeros((H, W), bool)
    tx, ty = np.float64(np.float32(tan_fov[0])), np.float64(np.float32(tan_fov[1]))
    xs, ys = np.arange(1, W - 1), np.arange(1, H - 1)
    rx, rxl, rxr = (ndc(xs + k, W, semantics, np.float64)[None, :] * tx for k in (0, -1, 1))
    ry, ryu, ryd = (ndc(ys + k, H, semantics, np.float64)[:, None] * ty for k in (0, -1, 1))
    du, dd, dl, dr = D[:-2, 1:-1], D[2:, 1:-1], D[1:-1, :-2], D[1:-1, 2:]
    with np.errstate(all="ignore"):
        ok = lambda d: np.isfinite(d) & (d > 0)
        finite = ok(du) & ok(dd) & ok(dl) & ok(dr)
        dv = np.stack(np.broadcast_arrays(rx * dd - rx * du, ryd * dd - ryu * du, dd - du))
        dh = np.stack(np.broadcast_arrays(rxr * dr - rxl * dl, ry * dr - ry * dl, dr - dl))
        c = np.cross(dv, dh, axis=0)
        dot = c[0] * rx + c[1] * ry + c[2]
        length = np.sqrt((c * c).sum(0))
        valid = finite & np.isfinite(length) & (length != 0)
        product = np.sqrt((dv * dv).sum(0) * (dh * dh).sum(0))
        close = (np.abs(dot) <= MARGIN * length * np.sqrt(rx * rx + ry * ry + 1.0)) | (length <= MARGIN * product)
    inner = (slice(1, -1), slice(1, -1))
    near[inner] = finite & close
    differ[inner] = ((finite != decisions["finite"][inner]) | (valid != decisions["valid"][inner])
                     | (valid & ((dot > 0) != decisions["flipped"][inner])))
    return near, differ


def consistency_pixels(drop, surface, tan_fov, semantics, decisions):
    """keep_n bool[H,W], the pixels that carry the normal-consistency term: the kept pixels (~drop) eroded by the
    4-neighbourhood — a dropped pixel's depth is a neighbour of four kept ones — without those on which a decision of the depth
    normal is near its threshold or differs from its float32 twin (depth_normal_pixels; surface: the float64 image)."""
    near, differ = depth_normal_pixels(surface, tan_fov, semantics, decisions)
    return eroded(~drop) & ~near & ~differ


def consistency_map(normal_map, depth, opacity_map, median_map, term, tan_fov, cut=None):
    """The map 1 - sum_c N_r N_d of normals.normal_consistency in torch: N_d = normals_ref.depth_normals64 of depth /
    opacity.clamp_min(1e-6) (term["surface"] == "median": of the median map) under term["decisions"], times opacity.detach()
    — or times term["opacity_weight"] [H,W], where the caller holds that constant factor at a value of its own."""
    from normals_ref import depth_normals64
    if term["surface"] == "median":
        surf = median_map
    else:
        surf = depth / (opacity_map.detach() if cut == "depth_normal_opacity" else opacity_map).clamp_min(1e-6)
    n_d = depth_normals64(surf, surf, surf, surf, tan_fov, term["semantics"], term["decisions"])
    if "opacity_weight" in term:                                 # (the detached factor held at a given value: finite differences)
        return 1.0 - (normal_map * n_d * torch.from_numpy(term["opacity_weight"]).to(n_d.dtype)).sum(0)
    n_d = n_d * (opacity_map if cut == "depth_normal_weight" else opacity_map.detach())
    return 1.0 - (normal_map * n_d).sum(0)


def gradients(leaf, structure, cam, w, wd, drop, dtype=F64, wf=None, wa=None, loss_terms=None, loss_only=False, **forward_options):
    """One step of the reference: forward(leaf, structure, <cam's tangents and size>, **forward_options), loss =
    (w . color).sum() + (wd . depth).sum() [+ (wf . feature_map).sum() + (wa . opacity_map).sum(): wf [C,H,W] with
    leaf["features"], wa [H,W] with opacity=True; afterwards aux["feature_map"] / ["opacity_map"] are float64 numpy] with the
    dropped pixels' weights zero, and autograd. A member of `leaf` that requires no gradient is a constant and has no entry. Returns (grads, color, depth,
    aux) — grads: float64 numpy, keyed by the leaves' names, by "means3D", "scales", "rotations", "opacities" (the gradients
    w.r.t. the activated arrays) and by "per_gaussian.mean2D" etc. (w.r.t. aux["per_gaussian"], rows in the order of
    aux["visible"]); zeros where the loss does not depend on the tensor.

    loss_terms: dict of the terms beyond the linear ones above, each optional (the GPU test builds the same with the library):
      "distortion": (lambda_d, g_d [H,W])   + lambda_d sum keep g_d distortion_map
      "median": g_m [H,W]                   + sum keep g_m median_map
      "normal_map": w_n [3,H,W]             + sum keep w_n normal_map
      "consistency": dict(weight=lambda_n, surface="expected" | "median", semantics=, decisions=, keep_n=)
                                            + lambda_n sum keep_n consistency_map(...): decisions, the depth normal's float32
                                            ones on the float32 maps; keep_n, consistency_pixels' (needs opacity=True)
    Afterwards aux["distortion_map"] / ["normal_map"] / ["median_map"] are float64 numpy too. loss_only=True returns the loss
    as a Python float instead, without differentiating."""
    depth = forward_options.get("depth", False)
    color, dmap, aux = forward(leaf, structure, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, **forward_options)
    keep = torch.from_numpy(~drop)
    wt, wdt = torch.from_numpy(w).to(dtype) * keep, torch.from_numpy(wd).to(dtype) * keep
    loss = (wt * color).sum() + ((wdt * dmap).sum() if depth else 0.0)
    if wf is not None:
        loss = loss + (torch.from_numpy(wf).to(dtype) * keep * aux["feature_map"]).sum()
    if wa is not None:
        loss = loss + (torch.from_numpy(wa).to(dtype) * keep * aux["opacity_map"]).sum()
    img = lambda a: torch.from_numpy(np.asarray(a)).to(dtype)
    terms = loss_terms or {}
    if "distortion" in terms:
        loss = loss + terms["distortion"][0] * (img(terms["distortion"][1]) * keep * aux["distortion_map"]).sum()
    if "median" in terms:
        loss = loss + (img(terms["median"]) * keep * aux["median_map"]).sum()
    if "normal_map" in terms:
        loss = loss + (img(terms["normal_map"]) * keep * aux["normal_map"]).sum()
    if "consistency" in terms:
        term = terms["consistency"]
        cmap = consistency_map(aux["normal_map"], dmap, aux["opacity_map"], aux.get("median_map"), term,
                               (cam.tan_fovx, cam.tan_fovy), forward_options.get("cut"))
        loss = loss + term["weight"] * (img(term["keep_n"]) * cmap).sum()
    if loss_only:                                                # (the float64 loss alone: for finite differences of it)
        return float(loss.detach())
    names = [k for k in leaf if leaf[k].requires_grad]
    tensors = [leaf[k] for k in names] + [aux[k] for k in ("means3D", "scales", "rotations", "opacities")]
    names = names + ["means3D", "scales", "rotations", "opacities"]
    for k, t in aux["per_gaussian"].items():
        if t is not None and t.requires_grad:
            names.append("per_gaussian." + k)
            tensors.append(t)
    got = torch.autograd.grad(loss, tensors, allow_unused=True)
    grads = {k: (g.detach().to(F64).numpy() if g is not None else np.zeros(tuple(t.shape)))
             for k, g, t in zip(names, got, tensors)}
    for k in ("feature_map", "opacity_map", "distortion_map", "normal_map", "median_map"):
        if aux.get(k) is not None:
            aux[k] = aux[k].detach().to(F64).numpy()
    return grads, color.detach().to(F64).numpy(), (dmap.detach().to(F64).numpy() if depth else None), aux
