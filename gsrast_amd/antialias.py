"""Antialiased splatting: the opacity compensation c = sqrt(det(cov2D) / det(cov2D + 0.3 I)) of upstream's `antialiasing`
switch (gsplat's rasterize_mode="antialiased", the 2D filter of Mip-Splatting), over gsr_antialias_forward / _backward
(include/gsrast_amd_antialias.h, csrc/antialias.hip).

gsr_forward dilates every projected covariance by 0.3 and uses the opacity unchanged; nothing of it but the blend looks at the
opacity. An antialiased frame is therefore the ordinary frame of the opacities o' = o * c:

  compensation   the plain call, for viewers: (o', c). Bind o' with SplatRasterizer.bind_scene and draw as usual.
  compensate     the same as a torch.autograd.Function, for trainers: what `rasterize(..., antialiased=True)` and
                 `render(..., antialiased=True)` put in front of the rasterizer.

This is the 2D half of Mip-Splatting; the other half, the 3D smoothing filter, is gsrast_amd/filter3d.py, whose smoothed
scales and opacities this pass then sees (`render(..., filter_3d=values, antialiased=True)`). What the mode is not: no
gradient reaches the camera through c — the view matrix is read, not differentiated; pose refinement in antialiased mode is
out of scope and refused.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi

F32 = torch.float32
_SEMANTICS = {"gscuda": 0, "inria": _capi.GSR_FLAG_SEMANTICS_INRIA}


def _rows(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if t.dtype != F32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return _capi.aligned16(t)


def _camera(view, proj, semantics: str, dev):
    if semantics not in _SEMANTICS:
        raise ValueError(f"semantics: {semantics!r} is not one of {sorted(_SEMANTICS)}")
    for name, m in (("view", view), ("proj", proj)):
        if m is None:
            continue
        if name == "view" and m.requires_grad:
            raise ValueError("view requires a gradient: the compensation reads the view matrix and does not differentiate it "
                             "(pose refinement in antialiased mode is not supported)")
        if m.dtype != F32 or m.numel() != 16 or m.device != dev:
            raise ValueError(f"{name}: expected 16 float32 values on {dev}, got {m.dtype} {tuple(m.shape)} on {m.device}")
    if proj is None and semantics != "inria":
        raise ValueError('proj is required with semantics="gscuda": that profile culls by the projected position')
    return view.detach().contiguous(), (proj.detach().contiguous() if proj is not None else None)


def _fill(a, n, means3D, scales, rotations, opacities, view, proj, tan_fov, width, height, semantics, scale_modifier, dev):
    a.struct_size = C.sizeof(type(a))
    a.flags = _SEMANTICS[semantics]
    a.num_gaussians, a.width, a.height = n, int(width), int(height)
    a.tan_fovx, a.tan_fovy, a.scale_modifier = float(tan_fov[0]), float(tan_fov[1]), float(scale_modifier)
    a.means3D, a.scales, a.rotations, a.opacities = means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(), opacities.data_ptr()
    a.view_matrix = view.data_ptr()
    a.proj_matrix = proj.data_ptr() if proj is not None else None
    a.stream = _capi.stream(dev)


def _inputs(means3D, scales, rotations, opacities):
    n = int(means3D.shape[0])
    return (n, _rows(means3D, (n, 4), "means3D"), _rows(scales, (n, 4), "scales"), _rows(rotations, (n, 4), "rotations"),
            _rows(opacities, (n,), "opacities"))


def compensation(means3D, scales, rotations, opacities, view, tan_fov, width, height, *, semantics: str = "gscuda",
                 scale_modifier: float = 1.0, proj=None):
    """(opacities_out [N], c [N]), new tensors: the compensated opacities o * c and the factor itself, for the camera
    (view, tan_fov = (tan_fovx, tan_fovy)) and a frame of width x height pixels, under `semantics` and `scale_modifier` as
    draw() takes them. means3D / scales / rotations [N,4], opacities [N]: float32 device tensors in the library's layouts;
    view (and proj): 16 floats on the device, column-major as Camera.view / .proj. proj is read by semantics="gscuda" only
    (its cull) and required there. One asynchronous launch on torch's current stream; no gradient is recorded.
    Forward-only use: `rast.bind_scene(means3D, scales, rotations, opacities_out, shs)` and draw."""
    dev = means3D.device
    view, proj = _camera(view, proj, semantics, dev)
    n, means3D, scales, rotations, opacities = _inputs(means3D.detach(), scales.detach(), rotations.detach(), opacities.detach())
    out, c = torch.empty((n,), dtype=F32, device=dev), torch.empty((n,), dtype=F32, device=dev)
    a = _capi.AntialiasArgs()
    _fill(a, n, means3D, scales, rotations, opacities, view, proj, tan_fov, width, height, semantics, scale_modifier, dev)
    a.opacities_out, a.compensation = out.data_ptr(), c.data_ptr()
    _capi.call("gsr_antialias_forward", C.byref(a), device=dev)
    return out, c


class _Compensate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, opacities, view, proj, opts):
        dev = means3D.device
        n, means3D, scales, rotations, opacities = _inputs(means3D, scales, rotations, opacities)
        out = torch.empty((n,), dtype=F32, device=dev)
        a = _capi.AntialiasArgs()
        _fill(a, n, means3D, scales, rotations, opacities, view, proj, dev=dev, **opts["call"])
        a.opacities_out = out.data_ptr()
        _capi.call("gsr_antialias_forward", C.byref(a), device=dev)
        ctx.opts, ctx.proj = opts, proj
        ctx.save_for_backward(means3D, scales, rotations, opacities, view)
        return out

    @staticmethod
    def backward(ctx, g_out):
        means3D, scales, rotations, opacities, view = ctx.saved_tensors
        opts, proj = ctx.opts, ctx.proj
        n, dev = int(means3D.shape[0]), means3D.device
        need_means, need_scales, need_rotations, need_opacities = ctx.needs_input_grad[:4]
        if g_out is None or not (need_means or need_scales or need_rotations or need_opacities):
            return (None,) * 7
        g_out = g_out.contiguous()                  # (rasterize hands over column 3 of dL_dconic_opacity: a strided view)
        assert g_out.dtype == F32 and tuple(g_out.shape) == (n,)
        slot = opts["radii_slot"]
        radii = slot.radii if slot is not None else None
        if radii is not None:
            assert radii.dtype == torch.int32 and tuple(radii.shape) == (n,) and radii.device == dev and radii.is_contiguous()
        new = lambda *shape: torch.empty(shape, dtype=F32, device=dev)
        d_means = new(n, 4) if need_means else None
        d_scales = new(n, 4) if need_scales else None
        d_rotations = new(n, 4) if need_rotations else None
        d_opacities = new(n) if need_opacities else None
        a = _capi.AntialiasBackwardArgs()
        _fill(a, n, means3D, scales, rotations, opacities, view, proj, dev=dev, **opts["call"])
        p = lambda t: t.data_ptr() if t is not None else None
        a.dL_dopacities_out, a.radii = g_out.data_ptr(), p(radii)
        a.dL_dopacities, a.dL_dmeans3D, a.dL_dscales, a.dL_drotations = p(d_opacities), p(d_means), p(d_scales), p(d_rotations)
        _capi.call("gsr_antialias_backward", C.byref(a), device=dev)
        return d_means, d_scales, d_rotations, d_opacities, None, None, None


def compensate(means3D, scales, rotations, opacities, view, tan_fov, width, height, *, semantics: str = "gscuda",
               scale_modifier: float = 1.0, proj=None, radii_slot=None):
    """The compensated opacities o * c [N] (a new tensor), differentiable: `compensation` with a backward. The backward is
    one kernel; it computes only the gradients of the inputs among means3D, scales, rotations and opacities that require
    one, and returns fresh tensors: dL/do = c * dL/do', and o * dL/do' taken through c to the mean, the scales and the
    rotation. radii_slot: an autograd.RadiiSlot that `rasterize` fills with the frame's radii; Gaussians the frame culled
    then get exact zeros without their rows being read (their dL/do' is zero anyway: they blended nothing).

    Raises ValueError if view requires a gradient: the gradient of c with respect to the camera is not computed, so pose
    refinement in antialiased mode is out of scope. (proj only decides the cull of semantics="gscuda": c does not vary with it.)"""
    dev = means3D.device
    view, proj = _camera(view, proj, semantics, dev)
    opts = {"radii_slot": radii_slot,
            "call": {"tan_fov": (float(tan_fov[0]), float(tan_fov[1])), "width": int(width), "height": int(height),
                     "semantics": semantics, "scale_modifier": float(scale_modifier)}}
    return _Compensate.apply(means3D, scales, rotations, opacities, view, proj, opts)
