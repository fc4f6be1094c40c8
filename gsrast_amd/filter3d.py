"""The 3D smoothing filter of Mip-Splatting (Yu et al., CVPR 2024), over gsr_filter3d_* (include/gsrast_amd_filter3d.h,
csrc/filter3d.hip): every Gaussian's size is bounded from below by the finest sampling rate a training camera saw it at, so
that a viewer moving closer than the training views sees no needle thinner than a training pixel.

  camera_records   cameras -> the 20-float records gsr_filter3d_observe reads, and the largest focal length
  Filter3D         the per-Gaussian filter values of a scene: observe (in batches) / finalize, compute = upstream's
                   compute_3D_filter, remap across a densification
  smoothed         the plain call, for viewers: (scales', opacities'). Bind them with SplatRasterizer.bind_scene.
  smooth           the same as a torch.autograd.Function, for trainers: what `render(..., filter_3d=values)` puts between
                   the activations and the rasterizer (in front of the 2D compensation of antialiased=True)
  save_fused_ply   upstream's save_fused_ply: a .ply whose scales and opacities are the smoothed ones

The training loop: `f.compute(params, cameras)` every 100 steps and after each densification (or `f.remap(src_of)` until
the next compute), and `render(params, rast, cam, filter_3d=f.values, antialiased=True)` in every step.

What is not upstream's: "never seen" is +inf, not a cap of 100000 with a flag array; the opacity coefficient is the product of
three ratios in [0, 1] instead of sqrt(det1 / det2), so extreme scales give no NaN; a filter value whose square is not
positive leaves the Gaussian untouched bit for bit; a scene no camera sees gets an all-zero filter where upstream raises;
and the screen-space dilation stays 0.3 (Mip-Splatting's rasterizer uses 0.1).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from .camera import Camera

F32 = torch.float32
CAMERA_FLOATS = _capi.GSR_FILTER3D_CAMERA_FLOATS


def camera_records(cameras):
    """(records float32 [C,20] (numpy), max_focal float): one record per camera in the order gsr_filter3d_observe reads —
    the three rows of the view matrix that produce t_0, t_1, t_2 (row 2 negated as Camera.view has it), f_x, f_y, W/2, H/2,
    -0.15 W, 1.15 W, -0.15 H, 1.15 H — and the largest f_x. cameras: Camera objects or tuples (view16, tan_fovx, tan_fovy,
    width, height), view16 column-major as Camera.view (an array or a tensor). f_x = W / (2 tan_fovx) and f_y = H / (2 tan_fovy)
    in float32; the four bounds are formed in double and rounded once."""
    f = np.float32
    out = np.zeros((len(cameras), CAMERA_FLOATS), np.float32)
    for k, cam in enumerate(cameras):
        if isinstance(cam, Camera):
            view, tan_x, tan_y, w, h = cam.view, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height
        else:
            view, tan_x, tan_y, w, h = cam
        if isinstance(view, torch.Tensor):
            view = view.detach().cpu().numpy()
        view = np.asarray(view, np.float32).reshape(-1)
        if view.size != 16 or int(w) <= 0 or int(h) <= 0 or not (float(tan_x) > 0.0 and float(tan_y) > 0.0):
            raise ValueError(f"camera {k}: expected 16 view floats, positive tangents and a positive size")
        w, h = int(w), int(h)
        out[k, 0:12] = view.reshape(4, 4).T[:3, :].reshape(12)        # V(r, c) = view[4 c + r]
        out[k, 12] = f(w) / (f(2.0) * f(tan_x))
        out[k, 13] = f(h) / (f(2.0) * f(tan_y))
        out[k, 14], out[k, 15] = f(w / 2.0), f(h / 2.0)
        out[k, 16], out[k, 17], out[k, 18], out[k, 19] = f(-0.15 * w), f(w * 1.15), f(-0.15 * h), f(1.15 * h)
    return out, (float(out[:, 12].max()) if len(cameras) else 0.0)


def _positions(xyz_or_params, n: int, dev):
    t = xyz_or_params.xyz if hasattr(xyz_or_params, "xyz") else xyz_or_params
    if not isinstance(t, torch.Tensor) or t.dtype != F32 or t.dim() != 2 or t.shape[0] != n or t.shape[1] not in (3, 4) or t.device != dev:
        raise ValueError(f"positions: expected float32 [{n}, 3 or 4] on {dev}, got "
                         f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    return t.detach().contiguous()


class Filter3D:
    """The filter values of a scene of n Gaussians on `device`. `values` (float32 [n]) is what `render(filter_3d=...)`,
    `smooth` and `smoothed` take: None until the first finalize(). Nothing here synchronises."""

    def __init__(self, n: int, device="cuda:0"):
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.values: "torch.Tensor | None" = None
        self.reset(int(n))

    def reset(self, n: "int | None" = None) -> None:
        """Forgets every observation (and the running max_focal); n: a new number of Gaussians. `values` stays as it is."""
        if n is not None:
            if n < 0:
                raise ValueError(f"n: {n}")
            self.n = int(n)
        self.min_depth = torch.full((self.n,), float("inf"), dtype=F32, device=self.device)
        self.max_focal = 0.0

    def observe(self, xyz_or_params, cameras) -> None:
        """Accumulates a batch of cameras (camera_records takes them) into min_depth: one launch. xyz_or_params: float32
        [n,3] (raw xyz) or [n,4] (means3D) on the device, or a GaussianParams."""
        pos = _positions(xyz_or_params, self.n, self.device)
        records, max_focal = camera_records(cameras)
        if len(cameras) == 0:
            return
        self.max_focal = max(self.max_focal, max_focal)
        rec = torch.from_numpy(records).to(self.device)
        a = _capi.Filter3dObserveArgs()
        a.struct_size, a.flags = C.sizeof(a), 0
        a.num_gaussians, a.position_stride, a.num_cameras = self.n, int(pos.shape[1]), int(rec.shape[0])
        a.positions, a.cameras, a.min_depth = pos.data_ptr(), rec.data_ptr(), self.min_depth.data_ptr()
        a.stream = _capi.stream(self.device)
        _capi.call("gsr_filter3d_observe", C.byref(a), device=self.device)

    def finalize(self) -> torch.Tensor:
        """values = (nearest depth / max_focal) * sqrt(0.2), a new tensor [n]; Gaussians no camera saw get the largest seen
        depth, and all zeros (no filter) if none was seen."""
        if not self.max_focal > 0.0:
            raise ValueError("finalize: no camera was observed")
        out = torch.empty((self.n,), dtype=F32, device=self.device)
        nbytes = int(_capi.lib().gsr_filter3d_temp_bytes(self.n))
        temp = torch.empty((max(nbytes, 16),), dtype=torch.uint8, device=self.device)
        a = _capi.Filter3dFinalizeArgs()
        a.struct_size, a.flags, a.num_gaussians, a.max_focal = C.sizeof(a), 0, self.n, self.max_focal
        a.min_depth, a.filter, a.temp, a.temp_bytes = self.min_depth.data_ptr(), out.data_ptr(), temp.data_ptr(), nbytes
        a.stream = _capi.stream(self.device)
        _capi.call("gsr_filter3d_finalize", C.byref(a), device=self.device)
        self.values = out
        return out

    def compute(self, xyz_or_params, cameras) -> torch.Tensor:
        """reset, observe, finalize: upstream's compute_3D_filter over `cameras`."""
        t = xyz_or_params.xyz if hasattr(xyz_or_params, "xyz") else xyz_or_params
        self.reset(int(t.shape[0]))
        self.observe(xyz_or_params, cameras)
        return self.finalize()

    def remap(self, src_of: torch.Tensor) -> torch.Tensor:
        """values[src_of]: carries the filter across densify_and_prune / add_new / prune_rows (row i of the new scene came
        from row src_of[i]) until the next compute(). The observations are reset to the new length."""
        if self.values is None:
            raise ValueError("remap: no values yet (finalize or compute first)")
        if src_of.dtype not in (torch.int32, torch.int64) or src_of.dim() != 1 or src_of.device != self.device:
            raise ValueError(f"src_of: expected int32 or int64 [M] on {self.device}, got {src_of.dtype} {tuple(src_of.shape)} on {src_of.device}")
        self.values = self.values[src_of.long()].contiguous()
        self.reset(int(src_of.shape[0]))
        return self.values


def _check(scales, opacities, filter_3d):
    n, dev = int(scales.shape[0]) if scales.dim() else -1, scales.device
    for name, t, shape in (("scales", scales, (n, 4)), ("opacities", opacities, (n,)), ("filter_3d", filter_3d, (n,))):
        if not isinstance(t, torch.Tensor) or t.dtype != F32 or tuple(t.shape) != shape or t.device != dev:
            raise ValueError(f"{name}: expected float32 {shape} on {dev}, got {getattr(t, 'dtype', type(t))} "
                             f"{tuple(getattr(t, 'shape', ()))} on {getattr(t, 'device', None)}")
    if filter_3d.requires_grad:
        raise ValueError("filter_3d requires a gradient: the filter is a constant (upstream's no_grad buffer)")
    return n, dev, _capi.aligned16(scales), opacities.contiguous(), filter_3d.contiguous()


def _forward(n, dev, scales, opacities, filter_3d, want_scales=True, want_opacities=True):
    s_out = torch.empty((n, 4), dtype=F32, device=dev) if want_scales else None
    o_out = torch.empty((n,), dtype=F32, device=dev) if want_opacities else None
    a = _capi.Filter3dArgs()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), 0, n
    a.scales, a.opacities, a.filter = scales.data_ptr(), opacities.data_ptr(), filter_3d.data_ptr()
    a.scales_out = s_out.data_ptr() if s_out is not None else None
    a.opacities_out = o_out.data_ptr() if o_out is not None else None
    a.stream = _capi.stream(dev)
    _capi.call("gsr_filter3d_forward", C.byref(a), device=dev)
    return s_out, o_out


def smoothed(scales, opacities, filter_3d):
    """(scales' [N,4], opacities' [N]), new tensors: s'_j = sqrt(s_j^2 + f^2) (the fourth float carried) and
    o' = o sqrt(prod_j s_j^2 / s'_j^2). scales [N,4], opacities [N], filter_3d [N]: float32 on one device, in the library's
    layouts. One asynchronous launch on torch's current stream; no gradient is recorded. Forward-only use:
    `rast.bind_scene(means3D, scales', rotations, opacities', shs)` and draw."""
    n, dev, scales, opacities, filter_3d = _check(scales.detach(), opacities.detach(), filter_3d)
    return _forward(n, dev, scales, opacities, filter_3d)


class _Smooth(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, opacities, filter_3d, radii_slot):
        n, dev, scales, opacities, filter_3d = _check(scales, opacities, filter_3d)
        s_out, o_out = _forward(n, dev, scales, opacities, filter_3d)
        ctx.radii_slot = radii_slot
        ctx.save_for_backward(scales, opacities, filter_3d)
        ctx.set_materialize_grads(False)
        need_scales, need_opacities = ctx.needs_input_grad[:2]
        if not need_scales:
            ctx.mark_non_differentiable(s_out)          # (s' depends on the scales alone)
        if not (need_scales or need_opacities):
            ctx.mark_non_differentiable(o_out)
        return s_out, o_out

    @staticmethod
    def backward(ctx, g_scales, g_opacities):
        scales, opacities, filter_3d = ctx.saved_tensors
        n, dev = int(scales.shape[0]), scales.device
        need_scales, need_opacities = ctx.needs_input_grad[:2]
        need_opacities = need_opacities and g_opacities is not None
        if (g_scales is None and g_opacities is None) or not (need_scales or need_opacities):
            return None, None, None, None
        if g_scales is not None:
            assert g_scales.dtype == F32 and tuple(g_scales.shape) == (n, 4)
            g_scales = _capi.aligned16(g_scales)
        if g_opacities is not None:
            assert g_opacities.dtype == F32 and tuple(g_opacities.shape) == (n,)
            g_opacities = g_opacities.contiguous()      # (rasterize hands over column 3 of dL_dconic_opacity: a strided view)
        slot = ctx.radii_slot
        radii = slot.radii if slot is not None else None
        if radii is not None:
            assert radii.dtype == torch.int32 and tuple(radii.shape) == (n,) and radii.device == dev and radii.is_contiguous()
        d_scales = torch.empty((n, 4), dtype=F32, device=dev) if need_scales else None
        d_opacities = torch.empty((n,), dtype=F32, device=dev) if need_opacities else None
        p = lambda t: t.data_ptr() if t is not None else None
        a = _capi.Filter3dBackwardArgs()
        a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), 0, n
        a.scales, a.opacities, a.filter = scales.data_ptr(), opacities.data_ptr(), filter_3d.data_ptr()
        a.dL_dscales_out, a.dL_dopacities_out, a.radii = p(g_scales), p(g_opacities), p(radii)
        a.dL_dscales, a.dL_dopacities = p(d_scales), p(d_opacities)
        a.stream = _capi.stream(dev)
        _capi.call("gsr_filter3d_backward", C.byref(a), device=dev)
        return d_scales, d_opacities, None, None


def smooth(scales, opacities, filter_3d, radii_slot=None):
    """(scales', opacities'), differentiable: `smoothed` with a backward. The backward is one kernel; it computes only the
    gradients of the inputs among scales and opacities that require one, and returns fresh tensors: dL/do = coef dL/do',
    and dL/ds from dL/ds' and, through coef, from o dL/do'. The filter is a constant. radii_slot: an autograd.RadiiSlot that
    `rasterize` fills with the frame's radii; Gaussians the frame culled then get exact zeros without their rows being read
    (the pass is elementwise: its gradient is zero wherever the rasterizer's is)."""
    return _Smooth.apply(scales, opacities, filter_3d, radii_slot)


def save_fused_ply(params, filter_3d, path: str) -> None:
    """Upstream's save_fused_ply: `params` written as a 3DGS .ply (ply.write_ply) whose scales and opacities are the smoothed
    ones, put back as log and logit, so that any 3DGS viewer — this library's load_ply included — shows the filtered scene."""
    from . import autograd as _autograd
    from . import ply as _ply
    with torch.no_grad():
        _, scales, _, opacities = params.activated()
        s, o = smoothed(scales, opacities, filter_3d)
        log_scale = torch.log(s[:, :3])
        logit = torch.log(o / (1.0 - o))
    host = lambda t: t.detach().cpu().numpy()
    sh = host(params.shs)
    if params.sh_layout == "coefficient_major":
        sh = _autograd._rest_to_file_order(sh)
    _ply.write_ply(path, host(params.xyz), sh, host(logit), host(log_scale), host(params.rotation))
