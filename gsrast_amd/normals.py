"""The two operators of the normal-consistency loss L_n = mean_p (1 - N_r(p) . N_d(p)) of 2DGS, GOF, RaDe-GS and PGSR, over
gsr_gaussian_normals_forward / _backward and gsr_depth_normals_forward / _backward (include/gsrast_amd_normals.h,
csrc/normals.hip):

  gaussian_normals     per-Gaussian normals [N,3]: the shortest axis of each Gaussian in view space, turned towards the camera.
                       Composited as three feature channels they are N_r: what `rasterize(..., normals=True)` and
                       `render(..., normals=True)` return as normal_map.
  depth_normals        the normal [3,H,W] of the surface a depth image [H,W] describes, from its four neighbours' points.
  normal_consistency   2DGS's term: the per-pixel map 1 - sum_c N_r N_d with N_d = depth_normals(depth / opacity) * opacity.

What is not differentiated: the per-Gaussian normal with respect to the scales (which axis is shortest is a decision), the mean
and the camera (they decide the flip; the view matrix is read) — its gradient goes to the rotations only; the depth normal with
respect to tan_fov.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi

F32 = torch.float32
_SEMANTICS = {"gscuda": 0, "inria": _capi.GSR_FLAG_SEMANTICS_INRIA}


def _flags(semantics: str) -> int:
    if semantics not in _SEMANTICS:
        raise ValueError(f"semantics: {semantics!r} is not one of {sorted(_SEMANTICS)}")
    return _SEMANTICS[semantics]


def _rows(t: torch.Tensor, shape, name: str) -> torch.Tensor:
    if t.dtype != F32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected float32 {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
    return _capi.aligned16(t)


def _fill_gaussians(a, n, means3D, scales, rotations, view, flags, dev):
    a.struct_size = C.sizeof(type(a))
    a.flags, a.num_gaussians = flags, n
    a.means3D, a.scales, a.rotations, a.view_matrix = means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(), view.data_ptr()
    a.stream = _capi.stream(dev)


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, scales, rotations, view, flags, radii_slot):
        n, dev = int(means3D.shape[0]), means3D.device
        means3D, scales, rotations = _rows(means3D, (n, 4), "means3D"), _rows(scales, (n, 4), "scales"), _rows(rotations, (n, 4), "rotations")
        out = torch.empty((n, 3), dtype=F32, device=dev)
        a = _capi.GaussianNormalsArgs()
        _fill_gaussians(a, n, means3D, scales, rotations, view, flags, dev)
        a.normals = out.data_ptr()
        _capi.call("gsr_gaussian_normals_forward", C.byref(a), device=dev)
        ctx.flags, ctx.slot = flags, radii_slot
        ctx.save_for_backward(means3D, scales, rotations, view)
        return out

    @staticmethod
    def backward(ctx, g):
        means3D, scales, rotations, view = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[2]:
            return (None,) * 6
        n, dev = int(means3D.shape[0]), means3D.device
        g = g.contiguous()                          # (rasterize hands over the last three columns of dL_dfeatures: a strided view)
        assert g.dtype == F32 and tuple(g.shape) == (n, 3)
        radii = ctx.slot.radii if ctx.slot is not None else None
        if radii is not None:
            assert radii.dtype == torch.int32 and tuple(radii.shape) == (n,) and radii.device == dev and radii.is_contiguous()
        d_rotations = torch.empty((n, 4), dtype=F32, device=dev)
        a = _capi.GaussianNormalsBackwardArgs()
        _fill_gaussians(a, n, means3D, scales, rotations, view, ctx.flags, dev)
        a.dL_dnormals, a.radii = g.data_ptr(), (radii.data_ptr() if radii is not None else None)
        a.dL_drotations = d_rotations.data_ptr()
        _capi.call("gsr_gaussian_normals_backward", C.byref(a), device=dev)
        return None, None, d_rotations, None, None, None


def gaussian_normals(means3D, scales, rotations, view, *, semantics: str = "gscuda", radii_slot=None):
    """Per-Gaussian normals [N,3] (a new tensor) in view space: column a of the profile's rotation matrix R, a the index of the
    smallest of the three scales, taken through the view matrix's 3 x 3 part, negated where it points away from the camera, and
    normalised; (0, 0, 0) where that length is zero or not finite. means3D / scales / rotations [N,4]: float32 device tensors in
    the library's layouts (the activated values: what `rasterize` takes); view: 16 floats on the device, column-major as
    Camera.view. The tensor is a `features` argument as it stands: SplatRasterizer.render_features of it is the normal map.

    Differentiable with respect to `rotations` only (one kernel, a fresh [N,4] tensor; under semantics="gscuda" through the
    normalisation of the quaternion too): the choice of the axis, the flip and the view matrix are the forward's decisions, and
    nothing goes to scales, means3D or the camera. radii_slot: an autograd.RadiiSlot that `rasterize` fills with the frame's radii;
    the backward passes them on if the slot has them by then, and Gaussians the frame culled get exact zeros without their rows
    being read.

    Raises ValueError if view requires a gradient: the normal is not differentiated with respect to the camera."""
    flags, dev = _flags(semantics), means3D.device
    if view.requires_grad:
        raise ValueError("view requires a gradient: the Gaussian normals read the view matrix and do not differentiate it "
                         "(pose refinement through the normal map is not supported)")
    if view.dtype != F32 or view.numel() != 16 or view.device != dev:
        raise ValueError(f"view: expected 16 float32 values on {dev}, got {view.dtype} {tuple(view.shape)} on {view.device}")
    return _GaussianNormals.apply(means3D, scales, rotations, view.detach().contiguous(), flags, radii_slot)


def _fill_depth(a, depth, tan_fov, flags, dev):
    a.struct_size = C.sizeof(type(a))
    a.flags, a.height, a.width = flags, int(depth.shape[0]), int(depth.shape[1])
    a.tan_fovx, a.tan_fovy = tan_fov
    a.depth = depth.data_ptr()
    a.stream = _capi.stream(dev)


class _DepthNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, tan_fov, flags):
        dev = depth.device
        depth = depth.contiguous()
        out = torch.empty((3,) + tuple(depth.shape), dtype=F32, device=dev)
        a = _capi.DepthNormalsArgs()
        _fill_depth(a, depth, tan_fov, flags, dev)
        a.normals = out.data_ptr()
        _capi.call("gsr_depth_normals_forward", C.byref(a), device=dev)
        ctx.tan_fov, ctx.flags = tan_fov, flags
        ctx.save_for_backward(depth)
        return out

    @staticmethod
    def backward(ctx, g):
        depth, = ctx.saved_tensors
        if g is None or not ctx.needs_input_grad[0]:
            return None, None, None
        dev = depth.device
        g = g.contiguous()
        assert g.dtype == F32 and tuple(g.shape) == (3,) + tuple(depth.shape)
        d_depth = torch.empty_like(depth)
        a = _capi.DepthNormalsBackwardArgs()
        _fill_depth(a, depth, ctx.tan_fov, ctx.flags, dev)
        a.dL_dnormals, a.dL_ddepth = g.data_ptr(), d_depth.data_ptr()
        _capi.call("gsr_depth_normals_backward", C.byref(a), device=dev)
        return d_depth, None, None


def depth_normals(depth, tan_fov, *, semantics: str = "gscuda"):
    """The normal [3,H,W] (a new tensor) of the surface the depth image [H,W] describes: depth is a view-space z per pixel, float32
    on the device; tan_fov = (tan_fovx, tan_fovy), Python floats; `semantics` chooses the profile's pixel-centre convention. A
    pixel's normal is the normalised cross product of the differences of its four neighbours' unprojected points, turned towards
    the camera; it is 0 on the one-pixel border, where a neighbour's depth is not finite or not positive, and where the cross
    product has no length. Differentiable with respect to `depth`: one gather kernel, no atomics, bit-reproducible."""
    flags = _flags(semantics)
    if depth.dtype != F32 or depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1 or not depth.is_cuda:
        raise ValueError(f"depth: expected float32 [H, W] on a device, got {depth.dtype} {tuple(depth.shape)} on {depth.device}")
    return _DepthNormals.apply(depth, (float(tan_fov[0]), float(tan_fov[1])), flags)


def normal_consistency(normal_map, depth_map, opacity_map, tan_fov, *, semantics: str = "gscuda", eps: float = 1e-6,
                       surface_depth=None):
    """2DGS's normal-consistency term as a per-pixel map [H,W]: 1 - sum_c N_r N_d, with N_r = normal_map [3,H,W] (the composited
    Gaussian normals: `render(..., normals=True)`) and N_d = depth_normals(depth_map / opacity_map.clamp_min(eps)) *
    opacity_map.detach() — the normal of the expected depth, weighted like N_r by the accumulated opacity. depth_map and
    opacity_map are `render(..., depth=True, opacity_grad=True)`'s. A torch composition around the fused operator: take `.mean()`
    for the loss.
    surface_depth: a depth image [H,W] to take the surface from instead — `render(..., median="depth")`'s median depth, 2DGS's
    depth_ratio = 1, which does not lie between surfaces at a silhouette as the expected depth does. N_d is then
    depth_normals(surface_depth) * opacity_map.detach(); depth_map is not read and may be None. The median depth is a step
    function of the geometry: through N_d the loss then reaches the means' z (and the view) only. The default, None, is the
    term as it was."""
    if surface_depth is not None:
        n_d = depth_normals(surface_depth, tan_fov, semantics=semantics) * opacity_map.detach()
    else:
        n_d = depth_normals(depth_map / opacity_map.clamp_min(eps), tan_fov, semantics=semantics) * opacity_map.detach()
    return 1.0 - (normal_map * n_d).sum(0)
