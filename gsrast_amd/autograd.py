"""torch.autograd over the rasterizer: raw (trainable) parameters -> image, and `loss.backward()` back to them.

  activate   raw parameters -> the arrays gsr_forward takes (gsr_activate_params / _backward, csrc/activations.hip)
  (filter3d.smooth   scales, opacities -> the 3D-filtered ones, between the two with filter_3d=values: gsrast_amd/filter3d.py)
  (antialias.compensate   opacities -> opacities * c, between the two with antialiased=True: gsrast_amd/antialias.py)
  (normals.gaussian_normals   scales, rotations -> three more feature channels, with normals=True: gsrast_amd/normals.py)
  rasterize  SplatRasterizer.draw / backward / camera_backward as one differentiable function
  GaussianParams, render   the two joined for a trainer: `render(params, rast, cam)` then `loss.backward()`

Ownership. Every tensor these functions return — images and gradients alike — is allocated by the call that returns it and
written by no later call of the library (the rasterizer writes into them through its `into=` arguments; nothing is cloned):
autograd may keep a gradient as `param.grad`, and a loss may be evaluated after the next frame was drawn. A
SplatRasterizer's chunks, on the other hand, hold ONE forward call: the backward of a frame must run before the same
rasterizer object draws again, and is refused (RuntimeError, nothing launched) if it did not. Keep one rasterizer object
per graph that is alive at the same time. (The median map of `median=` is the one exception: its backward holds the id map
and reads nothing of the frame.)
"""
from __future__ import annotations

import numpy as np
import torch

from . import _capi
from . import antialias as _antialias
from . import filter3d as _filter3d
from . import normals as _normals
from . import ply as _ply
from .camera import Camera
from .rasterizer import SplatRasterizer

F32 = torch.float32


def _f32c(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if t.dtype != F32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return _capi.aligned16(t)


class RadiiSlot:
    """Carries the radii of the frame from `rasterize` (which draws after `activate` ran) to the backward of `activate`:
    i32[N], a copy of the forward call's geomState.internal_radii; a Gaussian the frame culled then gets zero gradients
    without its rows being read."""

    def __init__(self):
        self.radii: "torch.Tensor | None" = None


class FrameSlot(RadiiSlot):
    """A RadiiSlot that also receives, in the frame's backward, dL_dmean2D [N,2]: the gradient w.r.t. each Gaussian's
    pixel-space centre (no NDC factor; a new tensor per frame) — the statistic densify.DensityStats.update() accumulates.
    The backward asks gsr_backward for one more array; the other gradients are the same bits as with a RadiiSlot.
    absgrad=True: the backward also calls SplatRasterizer.absgrad right behind gsr_backward, with the same three incoming
    gradients, and leaves abs_dL_dmean2D [N,2] (AbsGS's sum of absolute per-pixel shares, a new tensor per frame) here — what
    DensityStats.update(absgrad=True) takes. With the default nothing more is launched or allocated.
    With rasterize / render(features=...) dL_dmean2D includes the feature map's term (it is the gradient of the whole loss);
    abs_dL_dmean2D does not: it stays the score of the colour, depth and opacity terms. The same holds for the distortion
    map's term of rasterize / render(distortion=...)."""

    def __init__(self, absgrad: bool = False):
        super().__init__()
        self.absgrad = bool(absgrad)
        self.dL_dmean2D: "torch.Tensor | None" = None
        self.abs_dL_dmean2D: "torch.Tensor | None" = None


class _Activate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xyz, opacity_logit, log_scale, rotation, slot):
        n, dev = int(xyz.shape[0]), xyz.device
        xyz, log_scale, rotation = _f32c(xyz, (n, 3), "xyz"), _f32c(log_scale, (n, 3), "log_scale"), _f32c(rotation, (n, 4), "rotation")
        opacity_logit = _f32c(opacity_logit, (n,), "opacity_logit")
        means3D, scales, rotations = (torch.empty((n, 4), dtype=F32, device=dev) for _ in range(3))
        opacities = torch.empty((n,), dtype=F32, device=dev)
        _capi.call("gsr_activate_params", n, xyz.data_ptr(), opacity_logit.data_ptr(), log_scale.data_ptr(), rotation.data_ptr(),
                   means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(), opacities.data_ptr(), _capi.stream(dev), device=dev)
        ctx.save_for_backward(opacity_logit, log_scale, rotation)
        ctx.slot = slot
        # each output depends on one input: one whose input requires no gradient requires none either, and the rasterizer's
        # backward is then not asked for it
        need_xyz, need_opacity, need_scale, need_rotation = ctx.needs_input_grad[:4]
        off = [t for t, need in ((means3D, need_xyz), (scales, need_scale), (rotations, need_rotation), (opacities, need_opacity))
               if not need]
        if off:
            ctx.mark_non_differentiable(*off)
        return means3D, scales, rotations, opacities

    @staticmethod
    def backward(ctx, g_means, g_scales, g_rotations, g_opacities):
        opacity_logit, log_scale, rotation = ctx.saved_tensors
        n, dev = int(rotation.shape[0]), rotation.device
        want = [need and g is not None for need, g in zip(ctx.needs_input_grad[:4], (g_means, g_opacities, g_scales, g_rotations))]
        if not any(want):
            return None, None, None, None, None
        keep = []                                   # what the kernel reads must live until the launch is enqueued

        def vec4(g, name):
            g = _f32c(g, (n, 4), name)
            keep.append(g)
            return g.data_ptr()

        def opacity_vec4(g):
            """The opacity's gradient where the kernel reads it, in .w of a vec4 array: `rasterize` returns it as column 3
            of dL_dconic_opacity, which is then read in place; a plain [N] gradient is padded."""
            if (g.dtype == F32 and tuple(g.shape) == (n,) and n > 0 and g.stride(0) == 4 and g.storage_offset() >= 3
                    and (g.data_ptr() - 12) % 16 == 0):
                keep.append(g)
                return g.data_ptr() - 12
            t = torch.zeros((n, 4), dtype=F32, device=dev)
            t[:, 3] = g
            keep.append(t)
            return t.data_ptr()

        new = lambda *shape: torch.empty(shape, dtype=F32, device=dev)
        d_xyz = new(n, 3) if want[0] else None
        d_op = new(n) if want[1] else None
        d_scale = new(n, 3) if want[2] else None
        d_rot = new(n, 4) if want[3] else None
        radii = ctx.slot.radii if ctx.slot is not None else None
        if radii is not None:
            assert radii.dtype == torch.int32 and tuple(radii.shape) == (n,) and radii.device == dev and radii.is_contiguous()
        p = lambda t: t.data_ptr() if t is not None else None
        _capi.call(
            "gsr_activate_params_backward",
            n, p(opacity_logit) if want[1] else None, p(log_scale) if want[2] else None, p(rotation) if want[3] else None,
            p(radii), vec4(g_means, "dL_dmeans3D") if want[0] else None, vec4(g_scales, "dL_dscales") if want[2] else None,
            vec4(g_rotations, "dL_drotations") if want[3] else None, opacity_vec4(g_opacities) if want[1] else None,
            p(d_xyz), p(d_op), p(d_scale), p(d_rot), _capi.stream(dev), device=dev)
        return d_xyz, d_op, d_scale, d_rot, None


def activate(xyz, opacity_logit, log_scale, rotation, *, radii_slot: "RadiiSlot | None" = None):
    """Raw parameters -> (means3D [N,4] = (x,y,z,1), scales [N,4] = (exp s, e), rotations [N,4] = r/|r|, opacities [N] =
    sigmoid) on the device, in the float32 arithmetic of the .ply loader (bit-equal to `load_ply` of the same raw values).
    Inputs: float32 device tensors xyz [N,3], opacity_logit [N], log_scale [N,3], rotation [N,4] (real part first).
    Differentiable: the backward is one kernel, computes only the gradients of the inputs that require one, and returns
    fresh tensors. radii_slot: filled by `rasterize` with the frame's radii; culled Gaussians then get exact zeros. Pass
    one only when the rasterizer is the sole consumer of the four outputs (as `render` does): a regulariser on `scales`
    reaches culled Gaussians too. The opacity compensation of antialiased=True (antialias.compensate) is a second consumer
    that keeps the assumption: its gradient is exactly zero wherever the rasterizer's is, because dL/do' = 0 for a Gaussian
    that blended nothing. So does the 3D smoothing filter of filter_3d=values (filter3d.smooth), which stands between the two:
    the pass is elementwise, so its gradient is exactly zero wherever the gradients it receives are."""
    return _Activate.apply(xyz, opacity_logit, log_scale, rotation, radii_slot)


_DRAW_OPTIONS = ("plan", "overlap_emit", "tile_history", "deep_tiles")
STALE_MESSAGE = ("this rasterizer has drawn another frame, or was given another scene or camera, since the forward pass whose "
                 "backward is asked for: a SplatRasterizer holds the state of one forward call. Run backward() before the "
                 "same object renders again, or keep one rasterizer object per graph kept alive")


class _Rasterize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, features=None, distortion=None):
        n, dev = int(means3D.shape[0]), rast.device
        means3D, scales, rotations = _f32c(means3D, (n, 4), "means3D"), _f32c(scales, (n, 4), "scales"), _f32c(rotations, (n, 4), "rotations")
        opacities, shs = _f32c(opacities, (n,), "opacities"), _f32c(shs, (n, 48), "shs")
        if colors_precomp is not None:
            colors_precomp = _f32c(colors_precomp, (n, 3), "colors_precomp")
        rast.bind_scene(means3D, scales, rotations, opacities, shs)
        rast.set_camera_device(view, proj, cam_pos, *opts["tan_fov"])
        H, W, depth = rast.height, rast.width, opts["depth"]
        into = {"out_color": torch.empty((3, H, W), dtype=F32, device=dev)}
        if depth:
            into["out_depth"] = torch.empty((H, W), dtype=F32, device=dev)
        rast.draw(None, sync=False, semantics=opts["semantics"], sh_degree=opts["sh_degree"], scale_modifier=opts["scale_modifier"],
                  depth=depth, colors_precomp=colors_precomp if colors_precomp is not None else False, sorted_lists=True,
                  into=into, **opts["draw"])
        opacity_map = rast.opacity_map()                      # (1 - finalT: a new tensor)
        feature_map = None
        if features is not None:                              # (one more walk over the lists this draw() left; zero background)
            if features.dtype != F32 or features.dim() != 2 or int(features.shape[0]) != n or features.device != dev:
                raise ValueError(f"features: expected float32 [{n}, C] on {dev}, got {features.dtype} {tuple(features.shape)} on {features.device}")
            features = features.contiguous()
            feature_map = rast.render_features(features, sync=False)
        distortion_map = None
        if distortion is not None:                            # (likewise: gsr_distortion_forward; the moments go with this graph)
            if distortion.dtype != F32 or tuple(distortion.shape) != (n,) or distortion.device != dev:
                raise ValueError(f"distortion: expected float32 [{n}] on {dev}, got {distortion.dtype} {tuple(distortion.shape)} on {distortion.device}")
            distortion = distortion.contiguous()
            distortion_map = rast.render_distortion(distortion, power=opts["distortion_power"], sync=False)
            ctx.distortion_moments = rast._distortion_moments[2]
        if opts["radii_slot"] is not None:
            opts["radii_slot"].radii = rast.map_geometry_state()["radii"].clone()
        ctx.rast, ctx.opts = rast, opts
        ctx.receipt, ctx.epoch = rast.last_receipt.copy(), rast._state_epoch
        ctx.view_shapes = (view.shape, proj.shape, cam_pos.shape)
        ctx.has_colors = colors_precomp is not None
        ctx.has_features, ctx.has_distortion = features is not None, distortion is not None
        # (a write to one of them before backward() is reported)
        ctx.save_for_backward(means3D, scales, rotations, opacities, shs, *(t for t in (features, distortion) if t is not None))
        if not opts["opacity_grad"]:
            ctx.mark_non_differentiable(opacity_map)
        if opts["opacity_grad"] or features is not None or distortion is not None:
            ctx.set_materialize_grads(False)                  # (a map the loss does not use arrives as None, not as zeros to run through)
        return into["out_color"], into.get("out_depth"), opacity_map, feature_map, distortion_map

    @staticmethod
    def backward(ctx, g_color, g_depth, g_opacity_map, g_feature_map=None, g_distortion_map=None):
        rast, opts = ctx.rast, ctx.opts
        if rast._state_epoch != ctx.epoch:
            raise RuntimeError(STALE_MESSAGE)
        saved = ctx.saved_tensors                             # (raises if one was modified in place)
        need = dict(zip(("means3D", "scales", "rotations", "opacities", "shs", "view", "proj", "cam_pos", "colors_precomp", "features", "distortion"),
                        ctx.needs_input_grad[2:]))
        n, dev = rast.num_gaussians, rast.device
        g_alpha = g_opacity_map if opts["opacity_grad"] else None
        feature_term = (saved[5], g_feature_map) if (ctx.has_features and g_feature_map is not None) else None
        distortion_term = ((saved[6 if ctx.has_features else 5], g_distortion_map, opts["distortion_power"], ctx.distortion_moments)
                           if (ctx.has_distortion and g_distortion_map is not None) else None)
        if g_color is None and g_depth is None and g_alpha is None and feature_term is None and distortion_term is None:
            return (None,) * 13
        if g_color is None:
            g_color = torch.zeros((3, rast.height, rast.width), dtype=F32, device=dev)
        new = lambda *shape: torch.empty(shape, dtype=F32, device=dev)
        into = {}
        if need["means3D"]:
            into["dL_dmeans3D"] = new(n, 4)
        if need["scales"] or need["rotations"]:
            into["dL_dscales"] = new(n, 4)                   # (the chain writes the quaternion's gradient beside the scale's only)
        if need["rotations"]:
            into["dL_drotations"] = new(n, 4)
        if need["opacities"]:
            into["dL_dconic_opacity"] = new(n, 4)
        if need["shs"] and not ctx.has_colors:
            # the reference's colour reads the DC triple only: that chain writes floats 0..15 of a row, upstream's all 48
            into["dL_dshs"] = new(n, 48) if opts["semantics"] == "inria" else torch.zeros((n, 48), dtype=F32, device=dev)
        if need["means3D"] and opts["semantics"] == "inria" and not ctx.has_colors and "dL_dshs" not in into:
            into["dL_dshs"] = new(n, 48)                     # (gsr_backward forms dL_dmeans3D's term through the view direction with it)
        if need["colors_precomp"] and ctx.has_colors:
            into["dL_dcolors"] = new(n, 3)
        camera = need["view"] or need["proj"] or need["cam_pos"]
        if camera:
            into["camera"] = new(35)
        if not into:
            # nothing but the features requires a gradient: the frozen-geometry pass, no chain
            d_feat = (rast.features_backward(*feature_term, receipt=ctx.receipt, sync=False)
                      if (feature_term is not None and need["features"]) else None)
            d_val = (rast.distortion_backward(distortion_term[0], distortion_term[1], power=distortion_term[2], moments=distortion_term[3],
                                              receipt=ctx.receipt, sync=False)
                     if (distortion_term is not None and need["distortion"]) else None)
            return (None,) * 11 + (d_feat, d_val)
        frame_slot = opts["radii_slot"] if isinstance(opts["radii_slot"], FrameSlot) else None
        if frame_slot is not None:
            into["dL_dmean2D"] = new(n, 2)
        res = rast.backward(g_color, semantics=opts["semantics"], sh_degree=opts["sh_degree"], scale_modifier=opts["scale_modifier"],
                            receipt=ctx.receipt, wide_sums=True, dL_ddepth=g_depth if opts["depth"] else None,
                            depth=opts["depth"] or None, camera=camera, into=into, sync=False, dL_dalpha=g_alpha,
                            features=feature_term, distortion=distortion_term)
        if frame_slot is not None:
            frame_slot.dL_dmean2D = res["dL_dmean2D"]
            if frame_slot.absgrad:
                frame_slot.abs_dL_dmean2D = rast.absgrad(g_color, dL_ddepth=g_depth if opts["depth"] else None, depth=opts["depth"] or None,
                                                         dL_dalpha=g_alpha, receipt=ctx.receipt, semantics=opts["semantics"], sync=False)
        g = lambda k, on=True: res[k] if (on and k in res) else None
        cam_g = lambda k, name, shape: res[k].reshape(shape) if need[name] else None
        return (None, None, g("dL_dmeans3D"), g("dL_dscales", need["scales"]), g("dL_drotations"),
                res["dL_dconic_opacity"][:, 3] if need["opacities"] else None, g("dL_dshs", need["shs"]),
                cam_g("dL_dview_matrix", "view", ctx.view_shapes[0]), cam_g("dL_dproj_matrix", "proj", ctx.view_shapes[1]),
                cam_g("dL_dcam_pos", "cam_pos", ctx.view_shapes[2]), g("dL_dcolors"), g("dL_dfeatures", need["features"]),
                g("dL_dvalues", need["distortion"]))


def rasterize(rast: SplatRasterizer, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, tan_fov, *,
              semantics: str = "gscuda", sh_degree: int = 3, scale_modifier: float = 1.0, depth: "bool | str" = False,
              colors_precomp: "torch.Tensor | None" = None, radii_slot: "RadiiSlot | None" = None, opacity_grad: bool = False,
              antialiased: bool = False, features: "torch.Tensor | None" = None, distortion: "torch.Tensor | str | None" = None,
              distortion_power: int = 2, normals: bool = False, median: "torch.Tensor | str | None" = None,
              median_threshold: float = 0.5, **draw_options):
    """One differentiable frame: SplatRasterizer.draw forward, .backward / .camera_backward backward.

    Tensors in the library's layouts, float32 on rast.device: means3D / scales / rotations [N,4], opacities [N], shs [N,48]
    (as `semantics` reads them), view / proj (16 elements, column-major as Camera.view / .proj; any shape), cam_pos (3),
    colors_precomp [N,3] or None. tan_fov = (tan_fovx, tan_fovy), Python floats. The rasterizer is pointed at these tensors
    (bind_scene: nothing is copied) and the camera is copied on the device. draw_options: plan, overlap_emit, tile_history,
    deep_tiles, passed to draw(); the sorted lists are always written.

    Returns (color [3,H,W], depth [H,W] or None, opacity_map [H,W]), each a new tensor. opacity_map is the accumulated
    opacity 1 - finalT. opacity_grad=True makes it differentiable: its incoming gradient goes to gsr_backward_alpha as
    dL_dout_alpha (a seed of the render backward: no further sum, output or scratch), so depth / opacity_map.clamp_min(eps),
    a mask loss or an opacity regulariser reach every parameter and the camera. With the default, False, the map is marked
    non-differentiable: it carries no requires_grad, and dividing the depth channel by it treats it as a constant.

    The backward asks gsr_backward (double sums: the gradients do not depend on the order of the tiles' atomics) for exactly
    the per-Gaussian outputs whose input requires a gradient, written into new tensors; when view, proj or cam_pos requires
    one, it runs with camera=True and returns the three camera gradients in the inputs' shapes. With a FrameSlot as radii_slot
    it also asks for dL_dmean2D, into a new [N,2] tensor left in the slot, and a FrameSlot(absgrad=True) also gets abs_dL_dmean2D
    from one more pass (SplatRasterizer.absgrad). It raises RuntimeError
    before launching anything if `rast` drew again, or was rebound, after this call (see the module docstring).

    antialiased=True: upstream's `antialiasing`. The opacities pass through antialias.compensate first — o' = o * c with
    c = sqrt(det(cov2D) / det(cov2D + 0.3 I)), for the same semantics, scale_modifier, camera tensors, radii slot and the
    rasterizer's width and height — and the frame is the ordinary frame of o': the geometry chunk, the depth channel, the
    opacity map and gsr_contribution all see o'. Its backward adds c's gradients to the mean, the scales and the rotation.
    No gradient to the camera through c: a view that requires a gradient is a ValueError. (Mip-Splatting's 3D filter is
    `render`'s filter_3d, or filter3d.smooth on the scales and opacities handed in here.)

    features: float32 [N,C] on rast.device (1 <= C <= 256), which may require a gradient. The call then returns a 4-tuple,
    (color, depth, opacity_map, feature_map [C,H,W]): feature_map = sum_i features[i] alpha_i T_i with this frame's own alpha, T
    and decisions (SplatRasterizer.render_features), composited over a ZERO background — add (1 - opacity_map) * bg yourself,
    with opacity_grad=True if that term should reach the geometry. Its incoming gradient enters the same backward call as
    colour, depth and opacity (SplatRasterizer.backward(features=...)): the camera gradients, FrameSlot.dL_dmean2D,
    antialiased and the 3D filter all see the feature term. FrameSlot(absgrad=True)'s abs_dL_dmean2D does NOT include it.
    Without `features` the 3-tuple and everything about the call stay exactly as they were.

    distortion: a float32 [N] tensor on rast.device, one scalar m per Gaussian, which may require a gradient — or "depth": the
    view-space z of means3D, formed here with torch operations from means3D and view, so that its gradient flows back through
    torch to both. The distortion map [H,W] = sum_i sum_j w_i w_j |m_i - m_j|^distortion_power, w = alpha T of this frame
    (SplatRasterizer.render_distortion; the loss of Mip-NeRF 360 as 2DGS uses it; power 1 is signed in list order, which is the
    absolute form for the view depth), is then appended as the LAST element of the returned tuple: (color, depth, opacity_map[,
    feature_map], distortion_map). Its incoming gradient enters the same backward call as the other terms
    (SplatRasterizer.backward(distortion=...)), so the camera gradients, FrameSlot.dL_dmean2D, antialiased and the 3D filter
    all see it. FrameSlot(absgrad=True)'s abs_dL_dmean2D does NOT include it. Without `distortion` every return value and every
    launch stay as they were.

    normals=True: the per-Gaussian normals of normals.gaussian_normals — formed from the scales and rotations handed in here, for
    the same semantics, view tensor and radii slot — travel as three more channels of the ONE feature pass, behind the caller's
    `features` if any (C + 3 > 256 is a ValueError), and come back split off as normal_map [3,H,W], the alpha-blended view-space
    normals over a zero background: (color, depth, opacity_map[, feature_map], normal_map[, distortion_map]). Its incoming
    gradient enters the same backward call as the other terms and reaches every parameter the blend weights depend on and the
    camera through them; through the normals themselves it reaches the rotations only — not the scales, the means or the camera: a
    view that requires a gradient is a ValueError. With normals.depth_normals of depth / opacity_map it forms 2DGS's
    normal-consistency loss (normals.normal_consistency). Without `normals` every return value and every launch stay as they
    were.

    median: a float32 [N] tensor on rast.device, which may require a gradient — or "depth": the view-space z, formed exactly as
    distortion="depth" forms it. The median map [H,W] (SplatRasterizer.render_median: per pixel the value of the last blended
    record with a transmittance above median_threshold in front of it — 0.5: 2DGS's median depth; 0 where nothing was blended) is
    appended behind everything else, as the LAST element of the returned tuple. It is a STEP function of the geometry. What is not
    differentiated: the selection — the map's gradient reaches `median` only (SplatRasterizer.median_backward, the selection held
    fixed), and through torch, for "depth", means3D and the view; nothing reaches the scales, rotations or opacities through it.
    It is an autograd function of its own, called right behind the frame's: its backward holds the id map and nothing of the
    frame, so it also runs after `rast` has drawn again. Without `median` every return value and every launch stay as they
    were."""
    assert set(draw_options) <= set(_DRAW_OPTIONS), sorted(draw_options)
    assert depth in (False, True, "inverse"), depth
    opts = {"tan_fov": (float(tan_fov[0]), float(tan_fov[1])), "semantics": semantics, "sh_degree": int(sh_degree),
            "scale_modifier": float(scale_modifier), "depth": depth, "radii_slot": radii_slot, "draw": dict(draw_options),
            "opacity_grad": bool(opacity_grad), "distortion_power": int(distortion_power)}
    assert distortion_power in (1, 2), ("distortion_power", distortion_power)
    if antialiased:
        opacities = _antialias.compensate(means3D, scales, rotations, opacities, view, opts["tan_fov"], rast.width, rast.height,
                                          semantics=semantics, scale_modifier=opts["scale_modifier"], proj=proj, radii_slot=radii_slot)
    if median is not None:
        # (checked before anything is launched: the pass runs right behind the frame's own)
        median = _distortion_values(median, means3D, view)
        n = int(means3D.shape[0])
        if not isinstance(median, torch.Tensor) or median.dtype != F32 or tuple(median.shape) != (n,) or median.device != rast.device:
            raise ValueError(f"median: expected \"depth\" or float32 [{n}] on {rast.device}, got "
                             f"{getattr(median, 'dtype', type(median))} {tuple(getattr(median, 'shape', ()))}")
        median_threshold = float(median_threshold)
        if not 0.0 <= median_threshold < 1.0:
            raise ValueError(f"median_threshold: {median_threshold} is not in [0, 1)")
    if normals:
        res = _with_normals(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, features, distortion)
    elif distortion is None:
        if features is None:
            res = _Rasterize.apply(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, None, None)[:3]
        else:
            res = _Rasterize.apply(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, features, None)[:4]
    else:
        distortion = _distortion_values(distortion, means3D, view)
        out = _Rasterize.apply(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, features, distortion)
        res = out[:3] + ((out[3],) if features is not None else ()) + (out[4],)
    if median is None:
        return res
    return res + (_Median.apply(rast, median, median_threshold),)


class _Median(torch.autograd.Function):
    """The median map of the frame `rast` has just drawn (SplatRasterizer.render_median), differentiable with respect to the
    values with the selection held fixed. The backward holds the id map and nothing of the frame: it runs whether or not the
    rasterizer has drawn again, and _Rasterize knows nothing of it."""

    @staticmethod
    def forward(ctx, rast, values, threshold):
        res = rast.render_median(values, threshold=threshold, ids=True, sync=False)
        ctx.rast, ctx.ids, ctx.n = rast, res["ids"], rast.num_gaussians
        return res["map"]

    @staticmethod
    def backward(ctx, g):
        if g is None or not ctx.needs_input_grad[1]:
            return None, None, None
        rast = ctx.rast
        if rast.num_gaussians != ctx.n or tuple(ctx.ids.shape) != (rast.height, rast.width):
            raise RuntimeError("the rasterizer of this median map was given a scene or a frame of another size since it was rendered")
        return None, rast.median_backward(ctx.ids, g, sync=False), None


def _distortion_values(distortion, means3D, view):
    """rasterize's `distortion` (and `median`) as a tensor: "depth" is the view-space z of means3D, formed with torch operations."""
    if isinstance(distortion, str):
        assert distortion == "depth", distortion
        v = view.reshape(-1)                                  # (column-major: row 2 of the view matrix is elements 2, 6, 10, 14)
        distortion = (means3D[:, 0] * v[2] + means3D[:, 1] * v[6]) + (means3D[:, 2] * v[10] + v[14])
    return distortion


def _with_normals(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, features, distortion):
    """rasterize(normals=True): the Gaussian normals as the last three channels of the one feature pass, split off again."""
    n, dev = int(means3D.shape[0]), rast.device
    c = 0
    if features is not None:
        if features.dtype != F32 or features.dim() != 2 or int(features.shape[0]) != n or features.device != dev:
            raise ValueError(f"features: expected float32 [{n}, C] on {dev}, got {features.dtype} {tuple(features.shape)} on {features.device}")
        c = int(features.shape[1])
        if c + 3 > _capi.GSR_FEATURES_MAX_CHANNELS:
            raise ValueError(f"features: {c} channels and the three of normals=True are more than the feature pass's "
                             f"{_capi.GSR_FEATURES_MAX_CHANNELS}")
    per_gaussian = _normals.gaussian_normals(means3D, scales, rotations, view, semantics=opts["semantics"], radii_slot=opts["radii_slot"])
    channels = per_gaussian if features is None else torch.cat([features, per_gaussian], 1)
    if distortion is not None:
        distortion = _distortion_values(distortion, means3D, view)
    out = _Rasterize.apply(rast, opts, means3D, scales, rotations, opacities, shs, view, proj, cam_pos, colors_precomp, channels, distortion)
    return (out[:3] + ((out[3][:c],) if features is not None else ()) + (out[3][c:],)
            + ((out[4],) if distortion is not None else ()))


def _rest_to_coefficient_major(sh: np.ndarray) -> np.ndarray:
    """[N,48] in the file's order (f_dc 3, f_rest channel-major [3][15]) -> [N][16][3]."""
    n = sh.shape[0]
    out = sh.copy()
    out[:, 3:] = sh[:, 3:].reshape(n, 3, 15).transpose(0, 2, 1).reshape(n, 45)
    return out


def _rest_to_file_order(sh: np.ndarray) -> np.ndarray:
    n = sh.shape[0]
    out = sh.copy()
    out[:, 3:] = sh[:, 3:].reshape(n, 15, 3).transpose(0, 2, 1).reshape(n, 45)
    return out


class GaussianParams(torch.nn.Module):
    """The raw, trainable values of a scene: xyz [N,3], opacity_logit [N], log_scale [N,3], rotation [N,4] (unnormalised,
    real part first), shs [N,48] — what a 3DGS .ply stores and what an optimiser steps. sh_layout: "file" (f_rest
    channel-major, as stored; all the reference's semantics reads is the DC triple) or "coefficient_major" ([16][3], what
    semantics="inria" with sh_degree >= 1 reads)."""

    def __init__(self, xyz, opacity_logit, log_scale, rotation, shs, sh_layout: str = "file", device=None):
        super().__init__()
        assert sh_layout in ("file", "coefficient_major"), sh_layout
        self.sh_layout = sh_layout

        def param(a, shape):
            t = a.detach().clone() if isinstance(a, torch.Tensor) else torch.from_numpy(np.array(a, dtype=np.float32))
            t = t.to(device=device if device is not None else t.device, dtype=F32).reshape(shape).contiguous()
            return torch.nn.Parameter(t)
        n = int(np.shape(xyz)[0]) if not isinstance(xyz, torch.Tensor) else int(xyz.shape[0])
        self.xyz = param(xyz, (n, 3))
        self.opacity_logit = param(opacity_logit, (n,))
        self.log_scale = param(log_scale, (n, 3))
        self.rotation = param(rotation, (n, 4))
        self.shs = param(shs, (n, 48))

    @classmethod
    def from_raw(cls, xyz, opacity_logit, log_scale, rotation, shs, sh_layout: str = "file", device=None) -> "GaussianParams":
        """From arrays or tensors of raw values (copied); shs already in `sh_layout`."""
        return cls(xyz, opacity_logit, log_scale, rotation, shs, sh_layout, device)

    @classmethod
    def from_ply(cls, path: str, sh_layout: str = "file", device="cuda:0") -> "GaussianParams":
        """The file's raw values, unactivated (`activated()` of the result equals `ply.load_ply` of the file bit for bit)."""
        n, off = _ply.parse_header(path)
        raw = np.fromfile(path, dtype="<f4", offset=off, count=n * _ply.RECORD_FLOATS)
        if raw.size < n * _ply.RECORD_FLOATS:
            raise ValueError(f"{path}: file ends before {n} records")
        rec = raw.reshape(n, _ply.RECORD_FLOATS).astype(np.float32)
        sh = rec[:, 6:54]
        if sh_layout == "coefficient_major":
            sh = _rest_to_coefficient_major(sh)
        return cls(rec[:, 0:3], rec[:, 54], rec[:, 55:58], rec[:, 58:62], sh, sh_layout, device)

    @classmethod
    def from_points(cls, xyz, rgb, sh_layout: str = "file", device="cuda:0") -> "GaussianParams":
        """Initial Gaussians of a point cloud, as upstream's create_from_pcd makes them (init.initial_values): xyz [N,3]
        and rgb [N,3], arrays or tensors; rgb float in [0, 1], or uint8, which is divided by 255. The positions are
        checked once (one synchronisation, at initialisation): a non-finite one is a ValueError."""
        from . import init as _init
        dev = torch.device(device)

        def on_device(a, name):
            t = a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            if t.dim() != 2 or t.shape[1] != 3:
                raise ValueError(f"from_points: {name} is {tuple(t.shape)}, not [N, 3]")
            return t.to(dev)
        pos, col = on_device(xyz, "xyz"), on_device(rgb, "rgb")
        if col.shape[0] != pos.shape[0]:
            raise ValueError(f"from_points: {pos.shape[0]} positions and {col.shape[0]} colours")
        col = col.to(F32) / 255.0 if col.dtype == torch.uint8 else col.to(F32)
        pos = pos.to(F32).contiguous()
        if not bool(torch.isfinite(pos).all()):
            raise ValueError("from_points: a position is not finite")
        return cls(*_init.initial_values(pos, col), sh_layout, device)

    @classmethod
    def from_points_ply(cls, path: str, sh_layout: str = "file", device="cuda:0") -> "GaussianParams":
        """`from_points` of a points3D.ply (ply.read_points_ply)."""
        return cls.from_points(*_ply.read_points_ply(path), sh_layout, device)

    @property
    def num_gaussians(self) -> int:
        return int(self.xyz.shape[0])

    def activated(self, radii_slot: "RadiiSlot | None" = None):
        """(means3D, scales, rotations, opacities): `activate` of the raw values."""
        return activate(self.xyz, self.opacity_logit, self.log_scale, self.rotation, radii_slot=radii_slot)

    def save_ply(self, path: str) -> None:
        """Writes the raw values as a 3DGS .ply (ply.write_ply); a coefficient-major shs goes back to the file's order."""
        host = lambda t: t.detach().cpu().numpy()
        sh = host(self.shs)
        if self.sh_layout == "coefficient_major":
            sh = _rest_to_file_order(sh)
        _ply.write_ply(path, host(self.xyz), sh, host(self.opacity_logit), host(self.log_scale), host(self.rotation))


def _camera_tensors(camera, dev):
    if isinstance(camera, Camera):
        cache = camera.__dict__.setdefault("_device_tensors", {})
        key = str(dev)
        if key not in cache:
            cache[key] = tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32).reshape(-1).copy()).to(dev)
                               for a in (camera.view, camera.proj, camera.cam_pos))
        return cache[key] + (float(camera.tan_fovx), float(camera.tan_fovy))
    view, proj, cam_pos, tan_fovx, tan_fovy = camera
    return view, proj, cam_pos, float(tan_fovx), float(tan_fovy)


def render(params: GaussianParams, rast: SplatRasterizer, camera, *, semantics: str = "gscuda", sh_degree: int = 3,
           scale_modifier: float = 1.0, depth: "bool | str" = False, radii_slot: "RadiiSlot | None" = None,
           opacity_grad: bool = False, antialiased: bool = False, filter_3d: "torch.Tensor | None" = None,
           features: "torch.Tensor | None" = None, distortion: "torch.Tensor | str | None" = None, distortion_power: int = 2,
           normals: bool = False, median: "torch.Tensor | str | None" = None, median_threshold: float = 0.5, **draw_options):
    """`activate` then `rasterize`: (color [3,H,W], depth [H,W] or None, opacity_map [H,W]) of `params` seen from `camera`
    — a Camera (its matrices are uploaded once per device and kept with it; write to a Camera's arrays and it must be a new
    object) or a tuple (view, proj, cam_pos, tan_fovx, tan_fovy) whose first three are device tensors, which may require
    gradients. `loss.backward()` fills params.*.grad (and the camera tensors' .grad). Gaussians the frame culled get zero
    gradients without their rows being read. radii_slot: a RadiiSlot of the caller's, used instead of the call's own; after
    the call its `.radii` is the frame's radii (i32[N], a new tensor per frame) — what optim.GaussianAdam.step() takes. A
    FrameSlot also receives, in the backward, the frame's dL_dmean2D [N,2] — what densify.DensityStats.update() takes — and,
    as FrameSlot(absgrad=True), abs_dL_dmean2D [N,2], AbsGS's score, for DensityStats.update(absgrad=True).
    opacity_grad=True: the opacity map is differentiable too (see `rasterize`). antialiased=True: the opacities are
    compensated for the 0.3 dilation first (see `rasterize`); the view matrix must then not require a gradient.
    filter_3d: the 3D smoothing filter's values (filter3d.Filter3D.values: float32 [N] on the rasterizer's device, a constant),
    or None for none. The activated scales and opacities then pass through filter3d.smooth before anything else sees them —
    the rasterizer and, with antialiased=True, the 2D compensation, as in Mip-Splatting — and its backward takes the
    gradients back to the raw parameters. Another length, dtype or device is a ValueError.
    features: float32 [N,C] on the rasterizer's device (a Parameter of the caller's, say): the result is then the 4-tuple
    (color, depth, opacity_map, feature_map [C,H,W]) of `rasterize`, the feature map over a zero background.
    distortion, distortion_power: a float32 [N] tensor or "depth" (the view-space z): the distortion map [H,W] of `rasterize` is
    appended as the last element of the result.
    normals=True: the normal map [3,H,W] of `rasterize` — the per-Gaussian normals of the activated (and, with filter_3d, smoothed:
    the filter adds the same amount to every squared scale, so the shortest axis stays the shortest) scales and rotations — follows
    the feature map, before the distortion map; the view matrix must then not require a gradient.
    median, median_threshold: a float32 [N] tensor or "depth": the median map [H,W] of `rasterize` is appended as the last element
    of the result, behind the distortion map."""
    if semantics == "inria" and sh_degree >= 1:
        assert params.sh_layout == "coefficient_major", 'semantics="inria" reads shs as [N][16][3]: sh_layout="coefficient_major"'
    slot = radii_slot if radii_slot is not None else RadiiSlot()
    means3D, scales, rotations, opacities = params.activated(slot)
    if filter_3d is not None:
        scales, opacities = _filter3d.smooth(scales, opacities, filter_3d, radii_slot=slot)
    view, proj, cam_pos, tan_fovx, tan_fovy = _camera_tensors(camera, rast.device)
    return rasterize(rast, means3D, scales, rotations, opacities, params.shs, view, proj, cam_pos, (tan_fovx, tan_fovy),
                     semantics=semantics, sh_degree=sh_degree, scale_modifier=scale_modifier, depth=depth, radii_slot=slot,
                     opacity_grad=opacity_grad, antialiased=antialiased, features=features, distortion=distortion,
                     distortion_power=distortion_power, normals=normals, median=median, median_threshold=median_threshold,
                     **draw_options)
