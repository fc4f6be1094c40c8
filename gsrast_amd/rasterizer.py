"""Host side of the rasterizer: the role `GSGaussians` plays in the reference
(apps/gsrast/GSGaussians.cpp). PyTorch is used for device memory and streams only; every
stage runs in libgsrast_amd.so through the C ABI (include/gsrast_amd.h).

  ChunkBuffer            <-> resizeFunctional           (GSGaussians.cpp:27-42)
  SplatRasterizer.configure_from_scene <-> configureFromSplatData (:109-153)
  SplatRasterizer.draw   <-> GSGaussians::draw          (:155-212)
  SplatRasterizer.map_geometry_state <-> mapGeometryState (:214-219)
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi, backward_plan
from .backward_plan import DEPTHS, INTO, ROW_FLOATS, SET
from .camera import Camera


class ChunkBuffer:
    """Grow-only device chunk with 2x over-allocation, handed to the library as an
    allocator callback: `resizeFunctional` of the reference."""

    def __init__(self, device: torch.device):
        self.device = device
        self.tensor: torch.Tensor | None = None
        self.capacity = 0
        self.calls: list[int] = []          # sizes requested, in order (observable contract)
        self._cb = _capi.ALLOC_FN(self._alloc)

    def _alloc(self, _user, nbytes):
        self.calls.append(int(nbytes))
        try:
            if nbytes > self.capacity:
                self.tensor = None
                self.tensor = torch.empty(2 * int(nbytes), dtype=torch.uint8, device=self.device)
                self.capacity = 2 * int(nbytes)
            return self.tensor.data_ptr()
        except Exception:       # an exception must not cross the C boundary; NULL -> GSR_ERR_ALLOC
            return None

    @property
    def callback(self):
        return self._cb

    def base(self) -> int:
        return 0 if self.tensor is None else self.tensor.data_ptr()

    def view(self, ptr: int, count: int, dtype: torch.dtype) -> torch.Tensor:
        """Typed view of `count` elements starting at device address `ptr` inside the chunk."""
        off = ptr - self.base()
        nbytes = count * torch.empty((), dtype=dtype).element_size()
        assert 0 <= off and off + nbytes <= self.capacity, "state pointer outside its chunk"
        return self.tensor[off:off + nbytes].view(dtype)


def _dev(a, device, dtype=torch.float32) -> torch.Tensor:
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype).contiguous()


class BackwardBuffers:
    """The device memory one rasterizer's backward passes keep between calls, each piece created on first use.
      sets      per semantics, the arrays a call without into= hands out ({name: [N, k]}, backward_plan.output_set), rebuilt
                when with_cov3D changes. dL_dshs is 48 floats per Gaussian; the gscuda chain writes floats 0..15 of every
                row, the inria chain all 48: it is zero-filled once, and the sets are kept per semantics so that a gscuda
                call never returns what an inria call left in floats 16..47.
      scratch   by name, everything else: the arrays the camera pass reads where neither the caller nor a set has them,
                dL_ddepths (the only one a result names, and only without into=), sums_f64 [N,12] and depth_sums_f64 [N]
                (created zero, left zero by the library, never cleared here), camera_scratch, camera_grad (view | proj | cam_pos)."""

    def __init__(self, device: torch.device):
        self.device, self.n = device, 0
        self.sets: dict[str, dict[str, torch.Tensor]] = {}
        self.scratch: dict[str, torch.Tensor] = {}

    def fit(self, n: int) -> None:
        """The one rule for "N changed": all of this is sized by N, so all of it goes."""
        if n != self.n:
            self.n = n
            self.sets.clear()
            self.scratch.clear()

    def get(self, name: str, *shape, dtype=torch.float32) -> torch.Tensor:
        """scratch[name], created with `shape` on first use."""
        if name not in self.scratch:
            self.scratch[name] = torch.empty(shape, dtype=dtype, device=self.device)
        return self.scratch[name]

    def sums(self, name: str, *shape) -> torch.Tensor:
        """scratch[name] as the double sums of a pass: created zero, left zero by the library and never cleared here; a call
        that needs more of them than the one kept (a larger C) takes a new one. The caller drops it if its call fails."""
        t = self.scratch.get(name)
        if t is None or t.numel() < int(np.prod(shape)):
            t = self.scratch[name] = torch.zeros(shape, dtype=torch.float64, device=self.device)
        return t

    def take(self, plan: backward_plan.BackwardPlan, semantics: str, with_cov3D: bool, into: "dict | None") -> dict:
        """{name: tensor} of every array `plan` gives a pointer, each from the source the plan names."""
        own = None
        if plan.takes_output_set:
            own = self.sets.get(semantics)
            if own is None or ("dL_dcov3D" in own) != with_cov3D:
                own = self.sets[semantics] = {k: (torch.zeros if k == "dL_dshs" else torch.empty)(
                    (self.n, ROW_FLOATS[k]), dtype=torch.float32, device=self.device) for k in backward_plan.output_set(with_cov3D)}
        return {k: into[k] if source == INTO else own[k] if source == SET else
                self.get(k, *((self.n,) if k == DEPTHS else (self.n, ROW_FLOATS[k]))) for k, source in plan.sources.items()}


# gsr_forward_args.plan_used beside the plan's name: the attribute of the rasterizer that draw() sets from each bit
_PLAN_USED_FLAGS = (("last_blend_from_lists", _capi.GSR_PLAN_BLEND_FROM_LISTS),    # (block plan only: the blend read the sorted lists — sparse frames — instead of the block lists)
                    ("last_tiles_reordered", _capi.GSR_PLAN_TILES_REORDERED),
                    ("last_tile_order_dropped", _capi.GSR_PLAN_TILE_ORDER_DROPPED),
                    ("last_emit_overlapped", _capi.GSR_PLAN_EMIT_OVERLAPPED),
                    ("last_colors_beside", _capi.GSR_PLAN_COLORS_BESIDE),
                    ("last_deep_tiles", _capi.GSR_PLAN_DEEP_TILES))


class SplatRasterizer:
    """Uploads a scene once and renders it per camera through gsr_forward."""

    def __init__(self, width: int, height: int, device="cuda:0", background=(0.0, 0.0, 0.0)):
        self.lib = _capi.lib()                       # raises if the HIP library is missing
        if not torch.cuda.is_available():
            raise RuntimeError("SplatRasterizer needs a HIP device (no CPU fallback exists)")
        self.device = torch.device(device)
        self.width, self.height = int(width), int(height)
        self.geom = ChunkBuffer(self.device)
        self.binning = ChunkBuffer(self.device)
        self.image = ChunkBuffer(self.device)
        self.background = _dev(np.asarray(background, np.float32), self.device)
        self.out_color = torch.zeros((3, self.height, self.width), dtype=torch.float32, device=self.device)
        self.out_depth: torch.Tensor | None = None     # (H, W), allocated by the first draw(depth=...)
        self.last_depth: "bool | str" = False          # the depth mode of the last draw(): False, True or "inverse"
        self.num_gaussians = 0
        self.use_rects = True
        self.last_num_rendered = 0
        self.last_records_staged = 0
        self.last_plan = "none"
        for name, _ in _PLAN_USED_FLAGS:            # last_blend_from_lists, last_tiles_reordered, ...: of the last draw()
            setattr(self, name, False)
        self.last_lists_written = True
        self.last_receipt: _capi.ForwardReceipt | None = None      # of the last draw(): what backward() / poll take
        self.last_stage_ms: dict[str, float] = {}
        self.last_backward_ms: tuple = ()              # (render, chain) of the last backward(profile=True)
        self.last_camera_ms: "float | None" = None     # of the last camera_backward(profile=True)
        self.last_absgrad_ms: "float | None" = None    # of the last absgrad(profile=True)
        self.last_features_ms: "float | None" = None   # of the last render_features / features_backward / backward(features=...) with profile=True
        self.last_distortion_ms: "float | None" = None # of the last render_distortion / distortion_backward / backward(distortion=...) with profile=True
        self.last_median_ms: "float | None" = None     # of the last render_median / median_backward with profile=True
        # the moments of the last render_distortion: (that frame's receipt serial, the power, [3,H,W]) — what its backward reads
        self._distortion_moments: "tuple[int | None, int, torch.Tensor | None]" = (None, 0, None)
        self.rects: torch.Tensor | None = None
        self._bw = BackwardBuffers(self.device)
        # which colours a draw() composited (backward() reads the same ones): (that call's receipt serial, tensor or None)
        self._colors_of_call: "tuple[int | None, torch.Tensor | None]" = (None, None)
        self._means3: torch.Tensor | None = None       # draw_points' copy of the centres, three floats each
        # view (16) | proj (16) | cam_pos (3): one device buffer, uploaded with one async copy from pinned memory
        self._cam_dev = torch.zeros(35, dtype=torch.float32, device=self.device)
        self._cam_host = torch.zeros(35, dtype=torch.float32).pin_memory()
        self._view, self._proj, self._cam_pos = self._cam_dev[0:16], self._cam_dev[16:32], self._cam_dev[32:35]
        self._last_cam = None
        # counts what changes the state a backward pass reads (a draw, a camera upload, a new scene binding): what
        # gsrast_amd.autograd compares to refuse the backward of a frame that is no longer held
        self._state_epoch = 0
        # this view's tile history (gsr_tile_history: how long the tiles of its last frames took; the blend starts the slow
        # ones first). One per rasterizer object, so two of them on one thread do not feed each other's frames.
        self._history = C.c_void_p()
        _capi.call("gsr_tile_history_create", C.byref(self._history), device=self.device)

    _history = None             # (until __init__ has created it: __del__ also runs after an __init__ that raised)

    def __del__(self):
        h, self._history = self._history, None
        if h is not None and h.value:
            try:
                torch.cuda.synchronize(self.device)          # (the streams it was used on must be idle)
                self.lib.gsr_tile_history_destroy(h)
            except Exception:
                pass

    # -- scene upload -----------------------------------------------------------------
    def configure_from_scene(self, scene: dict, use_rects: bool = True) -> None:
        self.means3D = _dev(scene["means3D"], self.device)
        self.scales = _dev(scene["scales"], self.device)
        self.rotations = _dev(scene["rotations"], self.device)
        self.opacities = _dev(scene["opacities"], self.device)
        self.shs = _dev(scene["shs"], self.device)
        self.num_gaussians = int(self.means3D.shape[0])
        assert self.means3D.shape == (self.num_gaussians, 4) and self.scales.shape == (self.num_gaussians, 4)
        assert self.rotations.shape == (self.num_gaussians, 4) and self.shs.shape == (self.num_gaussians, 48)
        self.use_rects = use_rects
        self._colors_dc, self._colors_key = None, None   # colours precomputed from the DC triples, on first use, per SH tensor state
        self.rects = (torch.zeros((self.num_gaussians, 2), dtype=torch.int32, device=self.device)
                      if use_rects else None)
        self._state_epoch += 1

    def bind_scene(self, means3D: torch.Tensor, scales: torch.Tensor, rotations: torch.Tensor, opacities: torch.Tensor,
                   shs: torch.Tensor, use_rects: "bool | None" = None) -> None:
        """Points the rasterizer at the caller's device tensors (means3D / scales / rotations [N,4], opacities [N], shs
        [N,48]; float32, contiguous, on this device) without copying them: what a trainer whose activated parameters are new
        tensors every step calls per frame (gsrast_amd.autograd.rasterize does). `rects` is kept while N and use_rects
        (default: as it is) are unchanged; the precomputed-colour cache is dropped as configure_from_scene drops it."""
        n = int(means3D.shape[0])
        for name, t, shape in (("means3D", means3D, (n, 4)), ("scales", scales, (n, 4)), ("rotations", rotations, (n, 4)),
                               ("opacities", opacities, (n,)), ("shs", shs, (n, 48))):
            assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device, name
            assert tuple(t.shape) == shape and t.is_contiguous(), (name, tuple(t.shape), shape)
        self.means3D, self.scales, self.rotations, self.opacities, self.shs = means3D, scales, rotations, opacities, shs
        if use_rects is None:
            use_rects = self.use_rects
        if not use_rects:
            self.rects = None
        elif self.rects is None or self.rects.shape[0] != n:
            self.rects = torch.zeros((n, 2), dtype=torch.int32, device=self.device)
        self.use_rects = use_rects
        self.num_gaussians = n
        self._colors_dc, self._colors_key = None, None
        self._state_epoch += 1

    def set_camera(self, cam: Camera) -> None:
        """Uploads the 35 camera floats (the reference's caller copies view / proj per frame,
        GSGaussians.cpp:157-176). The same Camera object again is not re-uploaded."""
        assert cam.width == self.width and cam.height == self.height
        if cam is self._last_cam:
            return
        h = self._cam_host.numpy()
        h[0:16] = np.asarray(cam.view, np.float32).reshape(16)
        h[16:32] = np.asarray(cam.proj, np.float32).reshape(16)
        h[32:35] = np.asarray(cam.cam_pos, np.float32).reshape(3)
        self._cam_dev.copy_(self._cam_host, non_blocking=True)     # stream-ordered before the next forward call
        self._tan = (float(cam.tan_fovx), float(cam.tan_fovy))
        self._last_cam = cam
        self._state_epoch += 1

    def set_camera_device(self, view: torch.Tensor, proj: torch.Tensor, cam_pos: torch.Tensor, tan_fovx: float,
                          tan_fovy: float) -> None:
        """The 35 camera floats from device tensors (16 / 16 / 3 elements in the layouts of Camera.view / .proj / .cam_pos),
        copied on the device in stream order: no host round trip. A later set_camera uploads again, whichever Camera."""
        with torch.no_grad():
            for dst, src, k in ((self._view, view, 16), (self._proj, proj, 16), (self._cam_pos, cam_pos, 3)):
                assert isinstance(src, torch.Tensor) and src.device == self.device and src.numel() == k, (src.shape, k)
                dst.copy_(src.detach().reshape(k))
        self._tan = (float(tan_fovx), float(tan_fovy))
        self._last_cam = None
        self._state_epoch += 1

    # -- one frame --------------------------------------------------------------------
    def _forward_args(self, means3D: torch.Tensor, out_color: torch.Tensor) -> _capi.ForwardArgs:
        """gsr_forward_args as draw() and draw_points() both fill it; every other field is zero."""
        a = _capi.ForwardArgs()
        a.struct_size = C.sizeof(_capi.ForwardArgs)
        a.geometry_alloc, a.binning_alloc, a.image_alloc = self.geom.callback, self.binning.callback, self.image.callback
        a.num_gaussians, a.sh_dims, a.M = self.num_gaussians, 3, 16
        a.background = self.background.data_ptr()
        a.width, a.height = self.width, self.height
        a.means3D, a.shs = means3D.data_ptr(), self.shs.data_ptr()
        a.view_matrix, a.proj_matrix, a.cam_pos = self._view.data_ptr(), self._proj.data_ptr(), self._cam_pos.data_ptr()
        a.tan_fovx, a.tan_fovy = self._tan
        a.out_color = out_color.data_ptr()
        a.stream = _capi.stream(self.device)
        return a

    def draw(self, cam: Camera | None = None, *, profile: bool = False, count_staged: bool = False,
             tile_rows: tuple[int, int] | None = None, scale_modifier: float = 1.0,
             sync: bool = True, semantics: str = "gscuda", sh_degree: int = 3, plan: str = "auto",
             overlap_emit: "bool | None" = None, sorted_lists: bool = True, colors_precomp: "bool | torch.Tensor" = False,
             tile_history: "bool | str" = True, deep_tiles: "bool | str | None" = None,
             depth: "bool | str" = False, into: "dict | None" = None) -> torch.Tensor:
        """One `forward` call on the current torch stream. Returns the planar (3,H,W) image
        tensor owned by this object. `sync` adds the device synchronise the reference's caller
        performs after every call (CudaBuffer.hpp:8-12). semantics="inria" selects the upstream
        rasterizer's semantics (GSR_FLAG_SEMANTICS_INRIA): shs must then be laid out [N][16][3].
        plan: "auto" | "sort" | "blocks" — binning plan (GSR_FLAG_PLAN_*); the one used is in last_plan.
        overlap_emit: True = GSR_FLAG_OVERLAP_EMIT (block plan: the blend on a second stream beside the emission), False =
        GSR_FLAG_SERIAL_EMIT, None = the library decides per call (last_emit_overlapped tells).
        tile_history=False: GSR_FLAG_NO_TILE_HISTORY (the blend does not start the last frame's slowest tiles first); True: this
        object's own gsr_tile_history; "default": none passed — the library's own for the calling thread and stream (what a
        caller of the reference's signature gets); last_tile_order_dropped: the history's frames did not resemble each other.
        sorted_lists=False: GSR_FLAG_NO_SORTED_LISTS (forward-only callers; last_lists_written tells whether the
        binning chunk holds the sorted keys / values of this call).
        deep_tiles: None = the library decides per tile from the history (four waves for the tiles it expects to be the frame's
        slowest, csrc/blend.hip; last_deep_tiles tells whether the blend was launched with them enabled), False =
        GSR_FLAG_NO_DEEP_TILES, "all" = GSR_FLAG_DEEP_TILES_ALL (every tile; a diagnostic), "all8" / "all16" = eight / sixteen
        waves per tile (GSR_FLAG_DEEP_WAVES_8 / _16).
        colors_precomp: pass the scene's colours as the reference's `colorsPrecomp` argument (GSCuda.cuh:111) — computed once
        per scene by gsr_colors_from_dc, bit-equal to what the preprocess writes to geomState.rgb per frame (gscuda semantics
        only: there the colour does not depend on the view). A device tensor [N, 3] instead is passed as it is (any colours,
        either semantics); backward() then reads the same tensor.
        depth: True = also the depth channel (gsr_forward_args.out_depth: sum of z_i alpha_i T_i per pixel, view-space z, no
        background, not normalised — see opacity_map()), "inverse" = of 1 / z_i (GSR_FLAG_DEPTH_INVERSE); written to
        self.out_depth, an (H, W) tensor owned by this object.
        into: {"out_color": (3,H,W) tensor, "out_depth": (H,W) tensor} (either or both; float32, contiguous, on this device):
        the call writes the image / the depth channel there instead of into this object's own tensors, which it then leaves
        alone, and returns into["out_color"] if given — memory no later call of this object writes."""
        if cam is not None:
            self.set_camera(cam)
        self._state_epoch += 1
        out_color, out_depth = self.out_color, None
        if into is not None:
            assert set(into) <= {"out_color", "out_depth"}, sorted(into)
            for k, shape in (("out_color", (3, self.height, self.width)), ("out_depth", (self.height, self.width))):
                self._check_into(into.get(k), shape, k)
            out_color = into.get("out_color", out_color)
            out_depth = into.get("out_depth")
        a = self._forward_args(self.means3D, out_color)
        inria = semantics == "inria"
        assert semantics in ("gscuda", "inria")
        a.flags = ((_capi.GSR_FLAG_PROFILE if profile else 0) | (_capi.GSR_FLAG_COUNT_STAGED if count_staged else 0)
                   | (_capi.GSR_FLAG_SEMANTICS_INRIA if inria else 0)
                   | {"auto": 0, "sort": _capi.GSR_FLAG_PLAN_SORT, "blocks": _capi.GSR_FLAG_PLAN_BLOCKS}[plan]
                   | (_capi.GSR_FLAG_OVERLAP_EMIT if overlap_emit else (_capi.GSR_FLAG_SERIAL_EMIT if overlap_emit is False else 0))
                   | (0 if sorted_lists else _capi.GSR_FLAG_NO_SORTED_LISTS)
                   | (0 if tile_history else _capi.GSR_FLAG_NO_TILE_HISTORY)
                   | {"all": _capi.GSR_FLAG_DEEP_TILES_ALL, "all8": _capi.GSR_FLAG_DEEP_WAVES_8, "all16": _capi.GSR_FLAG_DEEP_WAVES_16,
                      False: _capi.GSR_FLAG_NO_DEEP_TILES, None: 0}[deep_tiles]
                   | (_capi.GSR_FLAG_DEPTH_INVERSE if depth == "inverse" else 0))
        assert depth in (False, True, "inverse"), depth
        if inria:
            a.sh_dims = sh_degree
        if isinstance(colors_precomp, torch.Tensor):
            assert colors_precomp.shape == (self.num_gaussians, 3) and colors_precomp.dtype == torch.float32
            assert colors_precomp.device == self.device and colors_precomp.is_contiguous()
            colors_used = colors_precomp
        else:
            assert not (colors_precomp and inria), "upstream colour depends on the view direction"
            colors_used = self.precomputed_colors() if colors_precomp else None
        a.colors_precomp = colors_used.data_ptr() if colors_used is not None else None
        a.opacities, a.scales = self.opacities.data_ptr(), self.scales.data_ptr()
        a.scale_modifier = scale_modifier
        a.rotations = self.rotations.data_ptr()
        a.rects = self.rects.data_ptr() if (self.rects is not None and not inria) else None
        a.tile_history = self._history if tile_history is True else None
        if depth:
            if out_depth is None:
                if self.out_depth is None:
                    self.out_depth = torch.zeros((self.height, self.width), dtype=torch.float32, device=self.device)
                out_depth = self.out_depth
            a.out_depth = out_depth.data_ptr()
        if tile_rows is not None:
            a.tile_row_begin, a.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        _capi.call("gsr_forward", C.byref(a), device=self.device)
        self.last_receipt = a.receipt.copy()
        self.last_colors_precomp = colors_used is not None
        self.last_depth = depth
        # which colours THIS call composited (backward() reads the same ones): tied to the call's receipt, not to "the last call"
        self._colors_of_call = (int(a.receipt.serial), colors_used)
        self.last_num_rendered = int(a.num_rendered)
        self.last_records_staged = int(a.records_staged)
        self.last_plan = _capi.PLAN_NAMES[int(a.plan_used) & 0xFF]
        self.last_lists_written = not (int(a.plan_used) & _capi.GSR_PLAN_LISTS_SKIPPED)
        for name, bit in _PLAN_USED_FLAGS:
            setattr(self, name, bool(int(a.plan_used) & bit))
        self.last_stage_ms = {n: float(a.stage_ms[i]) for i, n in enumerate(_capi.STAGE_NAMES)} if profile else {}
        if sync:
            torch.cuda.current_stream(self.device).synchronize()
            self.poll_async_error()
        return out_color

    def opacity_map(self) -> torch.Tensor:
        """(H, W) accumulated opacity of the last draw(), 1 - finalT: divide out_depth by it for expected depth. A gradient
        w.r.t. this map goes back through backward(dL_dalpha=...); under autograd, rasterize(opacity_grad=True)."""
        return 1.0 - self.map_image_state()["finalT"]

    def tile_history_stats(self) -> dict:
        """gsr_tile_history_stats of this object's history (host side; what the last sort of the blend's tile order found)."""
        out = (C.c_uint32 * 6)()
        _capi.call("gsr_tile_history_stats", self._history, out)
        return {"mean_ticks": int(out[0]), "longest_ticks": int(out[1]), "similarity": int(out[2]) / 1000.0,
                "order_dropped": bool(out[3]), "calls": int(out[4]), "overlapped": bool(out[5])}

    def tile_history_times(self):
        """(times, deep flags, deep count) of this object's history after its last call: numpy u32[tiles] in units of 10 ns,
        bool[tiles] (composited by four waves), and the number of deep tiles of the last sorted order (gsr_tile_history_times)."""
        tiles = ((self.width + 15) // 16) * ((self.height + 15) // 16)
        out, deep = (C.c_uint32 * tiles)(), C.c_uint32(0)
        _capi.call("gsr_tile_history_times", self._history, out, tiles, C.byref(deep))
        raw = np.frombuffer(out, dtype=np.uint32).copy()
        return raw & 0x7FFFFFFF, (raw >> 31).astype(bool), int(deep.value)

    def precomputed_colors(self) -> torch.Tensor:
        """vec3[N] = 0.5 + 0.4 DC (gsr_colors_from_dc), computed on first use and kept for the scene."""
        key = (self.shs.data_ptr(), self.shs._version)          # (callers may replace or write rast.shs between frames)
        if self._colors_dc is None or self._colors_key != key:
            c = torch.empty((self.num_gaussians, 3), dtype=torch.float32, device=self.device)
            _capi.call("gsr_colors_from_dc", self.num_gaussians, self.shs.data_ptr(), c.data_ptr(), _capi.stream(self.device),
                       device=self.device)
            self._colors_dc, self._colors_key = c, key
        return self._colors_dc

    def poll_async_error(self, receipt: "_capi.ForwardReceipt | None" = None) -> None:
        """After the stream of a draw() has been synchronised: raises if a device-side wait of that call gave up."""
        r = receipt if receipt is not None else self.last_receipt
        _capi.call("gsr_poll_async_error", C.byref(r), where="gsr_forward (device side)")

    # -- point-splat path (gscuda::forwardPoints, GSCuda.cu:110-155) -----------------------------
    def draw_points(self, cam: Camera | None = None, sync: bool = True) -> torch.Tensor:
        """One gsr_forward_points call: every centre lands on one pixel, the nearest wins. The image chunk
        then holds pc::ImageState (depth, temporary image); see map_points_image_state."""
        if cam is not None:
            self.set_camera(cam)
        self._state_epoch += 1
        if self._means3 is None or self._means3.shape[0] != self.num_gaussians:
            self._means3 = self.means3D[:, :3].contiguous()        # this path reads a stride of three floats
        a = self._forward_args(self._means3, self.out_color)
        _capi.call("gsr_forward_points", C.byref(a), device=self.device)
        if sync:
            torch.cuda.current_stream(self.device).synchronize()
        return self.out_color

    def map_points_image_state(self) -> dict:
        st = _capi.PointsImageState()
        P = self.width * self.height
        self.lib.gsr_points_image_from_chunk(self.image.base(), P, C.byref(st))
        v = self.image.view
        return {"depth": v(st.depth, P, torch.float32).view(self.height, self.width),
                "outColor": v(st.out_color, 3 * P, torch.float32).view(3, self.height, self.width)}

    # -- what the passes over a drawn frame share ---------------------------------------------
    def _map_frame(self, a, num_rendered: int) -> _capi.GeometryState:
        """Points the frame fields of the args struct `a` — those it has of means2D, conic_opacity, ranges, n_contrib, final_t
        and point_list — at what a forward call of `num_rendered` list entries left in the three chunks. Returns the geometry
        state, for the caller that takes more of it."""
        gst, ist, bst = _capi.GeometryState(), _capi.ImageState(), _capi.BinningState()
        self.lib.gsr_geometry_from_chunk(self.geom.base(), self.num_gaussians, C.byref(gst))
        self.lib.gsr_image_from_chunk(self.image.base(), self.width * self.height, C.byref(ist))
        self.lib.gsr_binning_from_chunk(self.binning.base(), num_rendered, C.byref(bst))
        frame = {"means2D": gst.means2D, "conic_opacity": gst.conic_opacity, "ranges": ist.ranges, "n_contrib": ist.n_contrib,
                 "final_t": ist.accum_alpha, "point_list": bst.values}
        for k, _ in a._fields_:
            if k in frame:
                setattr(a, k, frame[k])
        return gst

    def _walk_args(self, kind, rcpt: _capi.ForwardReceipt, tile_rows: "tuple[int, int] | None", profile: bool):
        """A gsr_features_args / gsr_distortion_args (`kind`) with the fields the two share, for the frame of `rcpt` on torch's
        current stream; the pass's own fields are left zero."""
        a = kind()
        a.struct_size = C.sizeof(kind)
        a.flags = _capi.GSR_FLAG_PROFILE if profile else 0
        a.num_gaussians, a.width, a.height = self.num_gaussians, self.width, self.height
        self._map_frame(a, int(rcpt.num_rendered))
        a.receipt = rcpt
        if tile_rows is None:                    # (the band the draw() itself had: the calls take no other)
            tile_rows = (int(rcpt.tile_row_begin), int(rcpt.tile_row_end))
        a.tile_row_begin, a.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        a.stream = _capi.stream(self.device)
        return a

    def _check_into(self, t: "torch.Tensor | None", shape: tuple, what=None) -> None:
        """A tensor of the caller's that the library is given as it stands (None: the caller gave none): float32, on this device,
        contiguous, exactly `shape`."""
        if t is None:
            return
        assert t.dtype == torch.float32 and t.device == self.device and t.is_contiguous(), what
        assert tuple(t.shape) == tuple(shape), (what, tuple(t.shape))

    def _new_output(self, rcpt: _capi.ForwardReceipt, tile_rows: "tuple[int, int] | None", shape: tuple) -> torch.Tensor:
        """A new per-pixel output of a pass: the call writes the rows of its band only — tile_rows, else the receipt's own band —
        so anything but the whole frame starts from zeros."""
        whole = tile_rows is None and (int(rcpt.tile_row_begin), int(rcpt.tile_row_end)) == (0, (self.height + 15) // 16)
        return (torch.empty if whole else torch.zeros)(shape, dtype=torch.float32, device=self.device)

    def _call(self, fn: str, a, *, drop: tuple = (), ms: "str | None" = None, sync: bool = False) -> None:
        """One library call on `a` with the tail the passes share: if it fails, the double sums named in `drop` go (a call that
        failed half way may have left sums behind: the next starts from zeroed ones); `ms` names the last_*_ms attribute that
        gets the call's stage_ms, None unless the call was profiled; sync waits for the stream."""
        try:
            _capi.call(fn, C.byref(a), device=self.device)
        except _capi.GsrError:
            for name in drop:
                self._bw.scratch.pop(name, None)
            raise
        if ms is not None:
            setattr(self, ms, float(a.stage_ms) if a.flags & _capi.GSR_FLAG_PROFILE else None)
        if sync:
            torch.cuda.current_stream(self.device).synchronize()

    def _check_dL_dalpha(self, dL_dalpha: "torch.Tensor | None") -> None:
        """backward()'s and absgrad()'s refusal of a dL_dalpha (checked before the first copy or launch of the call)."""
        if dL_dalpha is not None:
            assert isinstance(dL_dalpha, torch.Tensor) and dL_dalpha.dtype == torch.float32, "dL_dalpha: a float32 tensor"
            assert dL_dalpha.device == self.device, ("dL_dalpha", dL_dalpha.device, self.device)
            assert tuple(dL_dalpha.shape) == (self.height, self.width), ("dL_dalpha", tuple(dL_dalpha.shape))

    def _depth_gradient(self, dL_ddepth: "torch.Tensor | None", depth: "bool | str | None"):
        """(dL_ddepth as the library reads it, the depth channel's mode) of backward() and absgrad(); (None, None) without one."""
        if dL_ddepth is None:
            return None, None
        gd = dL_ddepth.to(device=self.device, dtype=torch.float32).contiguous()
        assert gd.shape == (self.height, self.width)
        return gd, backward_plan.depth_mode(depth, self.last_depth)

    # -- backward pass (BASELINE config 5; no counterpart in the reference) ------------------
    def _backward_args(self, rcpt: "_capi.ForwardReceipt | None", col: "torch.Tensor | None", semantics: str,
                       sh_degree: int) -> _capi.BackwardArgs:
        """gsr_backward_args with what does not depend on the gradients asked for: the scene, the camera and what the forward
        call of `rcpt` left in the three chunks (col: its precomputed colours, else its geomState.rgb)."""
        a = _capi.BackwardArgs()
        a.struct_size = C.sizeof(_capi.BackwardArgs)
        gst = self._map_frame(a, int(rcpt.num_rendered) if rcpt is not None else self.last_num_rendered)
        if semantics == "inria":
            a.flags = _capi.GSR_FLAG_SEMANTICS_INRIA
            a.cam_pos, a.shs, a.clamped, a.sh_dims = self._cam_pos.data_ptr(), self.shs.data_ptr(), gst.clamped, int(sh_degree)
        a.num_gaussians, a.width, a.height = self.num_gaussians, self.width, self.height
        a.background = self.background.data_ptr()
        a.cov3D, a.radii = gst.cov3D, gst.internal_radii
        a.colors = col.data_ptr() if col is not None else gst.rgb
        a.means3D, a.view_matrix = self.means3D.data_ptr(), self._view.data_ptr()
        a.tan_fovx, a.tan_fovy = self._tan
        a.stream = _capi.stream(self.device)
        if rcpt is not None:
            a.receipt = rcpt
        return a

    def backward(self, dL_dout: torch.Tensor, *, profile: bool = False, with_cov3D: bool = True,
                 tile_rows: tuple[int, int] | None = None, scale_modifier: float = 1.0, semantics: str = "gscuda",
                 sh_degree: int = 3, receipt: "_capi.ForwardReceipt | None | bool" = None, wide_sums: bool = True,
                 outputs: "tuple[str, ...] | None" = None, dL_ddepth: "torch.Tensor | None" = None,
                 depth: "bool | str | None" = None, camera: bool = False, into: "dict | None" = None,
                 sync: bool = True, dL_dalpha: "torch.Tensor | None" = None, features: "tuple | None" = None,
                 distortion: "tuple | None" = None) -> dict:
        """Gradients of sum(dL_dout * out_color) of the LAST draw() through gsr_backward; `semantics` / `sh_degree`
        must be those of that draw(). receipt: the gsr_forward_receipt of the draw() this is the backward of (default:
        this object's last draw(); any host thread may call); False = none, the reference's contract only (sorted lists
        in the binning chunk — refused after a draw(sorted_lists=False)). Returns device tensors dL_dmean2D [N,2], dL_dconic_opacity [N,4], dL_dcolors [N,3]
        and, with with_cov3D, dL_dcov2D [N,4] (m00, m01, m11, 0), dL_dcov3D [N,6], dL_dshs [N,48] (gscuda: the DC triple only; inria: every coefficient
        up to sh_degree), dL_dmeans3D / dL_dscales / dL_drotations [N,4].
        wide_sums: accumulate the per-Gaussian sums in double (gsr_backward_args.sums_f64: 96 N bytes of scratch kept by this
        object for as long as it lives — 0.56 GB for the 5.8 M-splat bench scene, 4.8 GB at 50 M; wide_sums=False does without
        it —, zero between calls and dropped if a call fails) — the gradients of screen-filling splats then no longer depend on the order in which the
        tiles' atomics arrive. outputs (needs wide_sums): the names to compute, e.g. BASELINE config 5's ("dL_dmean2D",
        "dL_dcov3D", "dL_dshs"); the others are neither computed nor written (the chain is bound by its writes) and
        absent from the result. The tensors are owned by this object and overwritten by the next call.
        dL_ddepth: (H, W) gradient w.r.t. the depth channel (gsr_backward_args.dL_dout_depth); the result then also holds
        dL_ddepths [N] (w.r.t. each Gaussian's d_i; one buffer for both semantics, which any later call with a depth gradient, into= or
        not, writes) and dL_dmeans3D includes the term through z. depth: the channel's mode,
        True or "inverse" (default: that of the last draw(depth=...), else True) — the backward recomputes d_i, so any
        draw() serves, whether or not it wrote out_depth.
        dL_dalpha: (H, W) float32 tensor on this device, the gradient w.r.t. the accumulated opacity 1 - finalT (opacity_map();
        gsr_backward_alpha of include/gsrast_amd_opacity.h). The loss gains sum(dL_dalpha * opacity_map) and every output receives its share
        (dL_dcolors none: the opacity does not depend on the colours); no further output, no further scratch. Another shape,
        dtype or device is refused (AssertionError) before anything is launched. For this term alone pass zeros as dL_dout.
        camera: the result also holds the gradients w.r.t. the camera, dL_dview_matrix (16,), dL_dproj_matrix (16,) and
        dL_dcam_pos (3,) in the layouts of Camera.view / .proj / .cam_pos (camera_backward(), right behind gsr_backward on the
        same stream). gsr_backward then also writes what that pass reads — dL_dmean2D, dL_dcov2D, and under inria with SH
        colours dL_dcolors — whatever `outputs` and `with_cov3D` say; arrays not asked for stay out of the result.
        into (needs wide_sums): {name: tensor} of the per-Gaussian outputs to compute, written into the caller's tensors
        (float32, contiguous, on this device, in the shapes above; with camera=True also "camera": (35,), view | proj |
        cam_pos) instead of this object's; it replaces `outputs`, and the result holds exactly these tensors (the camera's
        three as views of into["camera"]): memory no later call of this object writes. None of this object's output buffers
        is allocated for such a call; what the call needs beside them (dL_ddepths, the camera pass's inputs) is scratch
        of this object. dL_dshs under semantics="gscuda" must come zero-filled: that chain writes floats 0..15 of each row.
        sync=False: returns without waiting for the stream.
        features (needs wide_sums and a receipt): (F [N,C], dL_dfeature_map [C,H,W][, background [C]]) — the loss gains
        sum(dL_dfeature_map * render_features(F, background=...)). gsr_features_backward runs first, on the same stream, and adds
        the feature term's geometry sums into this object's sums_f64 scratch; gsr_backward / gsr_backward_alpha then chains the
        total, so every output (the camera's included) holds the feature term, and the result also holds dL_dfeatures [N,C], a
        new tensor. On an error both scratches are dropped. Without `features` the call is what it was.
        distortion (needs wide_sums and a receipt): (values [N], dL_ddistortion_map [H,W][, power = 2[, moments]]) — the loss gains
        sum(dL_ddistortion_map * render_distortion(values, power=power)); the moments are those that call kept (or the [3,H,W]
        tensor given), refused when they are of another frame or power. gsr_distortion_backward runs in front of gsr_backward,
        after the feature pass if both are given, and adds its geometry sums into the same sums_f64 scratch, so every output holds
        the term; the result also holds dL_dvalues [N], a new tensor. Without `distortion` the call is what it was."""
        n, dev = self.num_gaussians, self.device
        rcpt = self.last_receipt if receipt is None else (None if receipt is False else receipt)
        if distortion is not None:               # (checked before the first copy or launch of this call)
            assert wide_sums, "distortion= needs wide_sums: the distortion term reaches the chain through the sums_f64 scratch"
            assert rcpt is not None, "distortion= needs the receipt of a draw()"
            assert isinstance(distortion, (tuple, list)) and len(distortion) in (2, 3, 4), "distortion=(values, dL_ddistortion_map[, power[, moments]])"
            distortion_power = int(distortion[2]) if len(distortion) > 2 else 2
            assert distortion_power in (1, 2), ("power", distortion_power)
            distortion_moments = self._distortion_moments_of(rcpt, distortion_power, distortion[3] if len(distortion) > 3 else None)
        if features is not None:                 # (checked before the first copy or launch of this call)
            assert wide_sums, "features= needs wide_sums: the feature term reaches the chain through the sums_f64 scratch"
            assert rcpt is not None, "features= needs the receipt of a draw()"
            assert isinstance(features, (tuple, list)) and len(features) in (2, 3), "features=(F, dL_dfeature_map[, background])"
        col = self._colors_of(rcpt)
        plan = backward_plan.plan_backward(semantics, with_cov3D, wide_sums, None if outputs is None else tuple(outputs),
                                           None if into is None else tuple(into), dL_ddepth is not None, camera, col is not None)
        self._check_dL_dalpha(dL_dalpha)
        g = dL_dout.to(device=dev, dtype=torch.float32).contiguous()
        assert g.shape == (3, self.height, self.width)
        for k, t in (into or {}).items():
            if k != "camera":
                self._check_into(t, (n, ROW_FLOATS[k]), k)
        gd, mode = self._depth_gradient(dL_ddepth, depth)
        self._bw.fit(n)
        arrays = self._bw.take(plan, semantics, with_cov3D, into)
        a = self._backward_args(rcpt, col, semantics, sh_degree)
        a.flags |= (_capi.GSR_FLAG_PROFILE if profile else 0) | (_capi.GSR_FLAG_DEPTH_INVERSE if mode == "inverse" else 0)
        a.dL_dout_color = g.data_ptr()
        if dL_ddepth is not None:
            a.dL_dout_depth = gd.data_ptr()
        for k, t in arrays.items():             # (the fields of gsr_backward_args carry the arrays' names)
            setattr(a, k, t.data_ptr())
        if wide_sums:
            a.sums_f64 = self._bw.sums("sums_f64", n, 12).data_ptr()
            if dL_ddepth is not None:
                a.depth_sums_f64 = self._bw.sums("depth_sums_f64", n).data_ptr()
        if plan.chain_inputs:
            a.proj_matrix, a.scales, a.rotations = self._proj.data_ptr(), self.scales.data_ptr(), self.rotations.data_ptr()
            a.scale_modifier = scale_modifier
        if tile_rows is not None:
            a.tile_row_begin, a.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        feature_call = None
        if features is not None:
            feature_call, feature_keep = self._features_call(rcpt, features[0], features[2] if len(features) > 2 else None,
                                                             dL_dout=features[1], tile_rows=tile_rows, profile=profile)
        distortion_call = None
        if distortion is not None:
            distortion_call, distortion_keep = self._distortion_call(rcpt, distortion[0], distortion_power, distortion_moments,
                                                                     dL_dout=distortion[1], tile_rows=tile_rows, profile=profile)
        try:
            if feature_call is not None:        # its geometry sums go where gsr_backward's go: that call chains the total
                feature_call.geometry_sums_f64 = a.sums_f64
                _capi.call("gsr_features_backward", C.byref(feature_call), device=dev)
            if distortion_call is not None:     # (likewise; both passes may seed the same sums)
                distortion_call.geometry_sums_f64 = a.sums_f64
                _capi.call("gsr_distortion_backward", C.byref(distortion_call), device=dev)
            if dL_dalpha is None:
                _capi.call("gsr_backward", C.byref(a), device=dev)
            else:
                ga = dL_dalpha.contiguous()
                _capi.call("gsr_backward_alpha", C.byref(a), ga.data_ptr(), device=dev)
        except _capi.GsrError:
            if wide_sums:                        # (a call that failed half way may have left sums behind: the next starts from zeroed ones)
                self._bw.scratch.pop("sums_f64", None)
                self._bw.scratch.pop("depth_sums_f64", None)
            self._bw.scratch.pop("feature_sums_f64", None)
            self._bw.scratch.pop("distortion_sums_f64", None)
            raise
        self.last_backward_ms = (float(a.stage_ms[0]), float(a.stage_ms[1])) if profile else ()
        if feature_call is not None:
            self.last_features_ms = float(feature_call.stage_ms) if profile else None
            arrays["dL_dfeatures"] = feature_keep[-1]
        if distortion_call is not None:
            self.last_distortion_ms = float(distortion_call.stage_ms) if profile else None
            arrays["dL_dvalues"] = distortion_keep[-1]
        if camera:
            arrays.update(self.camera_backward({k: arrays[k] for k in plan.camera_inputs}, semantics=semantics,
                                               sh_degree=sh_degree, shs_colour="dL_dcolors" in plan.camera_inputs, depth=mode,
                                               profile=profile, sync=False, into=into["camera"] if plan.camera_into else None))
        if sync:
            torch.cuda.current_stream(dev).synchronize()
        return {k: arrays[k] for k in tuple(plan.result) + (("dL_dfeatures",) if feature_call is not None else ())
                + (("dL_dvalues",) if distortion_call is not None else ())}

    # -- N-channel feature maps (include/gsrast_amd_features.h) -------------------------------
    def _features_call(self, rcpt: _capi.ForwardReceipt, features: torch.Tensor, background, *, out: "torch.Tensor | None" = None,
                       dL_dout: "torch.Tensor | None" = None, into: "torch.Tensor | None" = None,
                       tile_rows: "tuple[int, int] | None" = None, profile: bool = False):
        """(gsr_features_args, the tensors it points at) for the frame of `rcpt`: the forward call's with `out`, the backward
        call's with dL_dout — the last tensor of the list is then dL_dfeatures (`into`, or a new one), and the double scratch
        is this object's (created zero, left zero by the library)."""
        n, dev = self.num_gaussians, self.device
        assert isinstance(features, torch.Tensor) and features.dtype == torch.float32 and features.device == dev, "features: a float32 tensor on this device"
        assert features.dim() == 2 and features.shape[0] == n, ("features", tuple(features.shape), n)
        c = int(features.shape[1])
        f = features.detach().contiguous()
        keep = [f]
        a = self._walk_args(_capi.FeaturesArgs, rcpt, tile_rows, profile)
        a.channels, a.features = c, f.data_ptr()
        if background is not None:
            bg = _dev(background, dev).reshape(-1)
            assert bg.numel() == c, ("background", tuple(bg.shape), c)
            keep.append(bg)
            a.background = bg.data_ptr()
        if out is not None:
            a.out = out.data_ptr()
            keep.append(out)
        if dL_dout is not None:
            g = dL_dout.to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(g.shape) == (c, self.height, self.width), ("dL_dfeature_map", tuple(g.shape))
            self._check_into(into, (n, c))
            res = into if into is not None else torch.empty((n, c), dtype=torch.float32, device=dev)
            self._bw.fit(n)
            a.dL_dout, a.dL_dfeatures = g.data_ptr(), res.data_ptr()
            a.feature_sums_f64 = self._bw.sums("feature_sums_f64", n * c).data_ptr()
            keep += [g, res]
        return a, keep

    def render_features(self, features: torch.Tensor, *, background=None, receipt: "_capi.ForwardReceipt | None" = None,
                        tile_rows: "tuple[int, int] | None" = None, into: "torch.Tensor | None" = None, profile: bool = False,
                        sync: bool = True) -> torch.Tensor:
        """[C,H,W]: sum_i features[i] alpha_i T_i per pixel of the last draw() (gsr_features_forward), with that call's own
        alpha, T and decisions — call it after a draw() and before the next one, as ContributionStats.update is used.
        features: float32 [N,C] on this device, 1 <= C <= 256. background: C floats composited behind (final_t * background),
        or None for none. With the frame's colours and background the result is out_color bit for bit. receipt: default this
        object's last draw(). tile_rows: the band to write, which must be that of the draw() (the default: the receipt's own rows);
        other rows are left alone. into: a float32 [C,H,W] tensor on this device, contiguous, written and returned; else a new
        tensor, zeros outside the band (all zeros for an empty band).
        One more walk over the sorted lists (refused after draw(sorted_lists=False)). profile: last_features_ms gets the time."""
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "render_features needs the receipt of a draw()"
        assert isinstance(features, torch.Tensor) and features.dim() == 2, "features: [N,C]"
        shape = (int(features.shape[1]), self.height, self.width)
        self._check_into(into, shape)
        out = into if into is not None else self._new_output(rcpt, tile_rows, shape)
        a, _keep = self._features_call(rcpt, features, background, out=out, tile_rows=tile_rows, profile=profile)
        self._call("gsr_features_forward", a, ms="last_features_ms", sync=sync)
        return out

    def features_backward(self, features: torch.Tensor, dL_dout: torch.Tensor, *, background=None,
                          receipt: "_capi.ForwardReceipt | None" = None, tile_rows: "tuple[int, int] | None" = None,
                          into: "torch.Tensor | None" = None, profile: bool = False, sync: bool = True) -> torch.Tensor:
        """dL_dfeatures [N,C] of sum(dL_dout * render_features(features)) for the last draw() (gsr_features_backward with no
        geometry sums: the frozen-geometry case — nothing else is computed and no scratch shared with backward() is touched;
        for the geometry's gradients too, pass features= to backward()). dL_dout: [C,H,W]. `background` does not enter this
        gradient and is accepted for symmetry. The scratch (8 N C bytes of doubles) is kept by this object, zero between calls
        and dropped if a call fails. into: a float32 [N,C] tensor on this device, contiguous, written in full and returned."""
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "features_backward needs the receipt of a draw()"
        a, keep = self._features_call(rcpt, features, background, dL_dout=dL_dout, into=into, tile_rows=tile_rows, profile=profile)
        self._call("gsr_features_backward", a, drop=("feature_sums_f64",), ms="last_features_ms", sync=sync)
        return keep[-1]

    # -- the depth distortion map (include/gsrast_amd_distortion.h) ---------------------------
    def _distortion_moments_of(self, rcpt: _capi.ForwardReceipt, power: int, moments: "torch.Tensor | None") -> torch.Tensor:
        """The [3,H,W] moments a backward call reads: `moments`, or those the last render_distortion of this frame and power left."""
        if moments is None:
            serial, kept_power, kept = self._distortion_moments
            assert kept is not None and serial == int(rcpt.serial) and kept_power == power, (
                "distortion: the moments kept by this rasterizer are stale — they are those of render_distortion for another "
                "frame or power (or there are none): call render_distortion(values, power=...) for this draw() first")
            moments = kept
        self._check_into(moments, (3, self.height, self.width), "moments")
        return moments

    def _distortion_call(self, rcpt: _capi.ForwardReceipt, values: torch.Tensor, power: int, moments: torch.Tensor, *,
                         out: "torch.Tensor | None" = None, dL_dout: "torch.Tensor | None" = None,
                         into: "torch.Tensor | None" = None, tile_rows: "tuple[int, int] | None" = None, profile: bool = False):
        """(gsr_distortion_args, the tensors it points at) for the frame of `rcpt`: the forward call's with `out`, the backward
        call's with dL_dout — the last tensor of the list is then dL_dvalues (`into`, or a new one), and the double scratch is
        this object's (created zero, left zero by the library)."""
        n, dev = self.num_gaussians, self.device
        assert isinstance(values, torch.Tensor) and values.dtype == torch.float32 and values.device == dev, "values: a float32 tensor on this device"
        assert values.dim() == 1 and values.shape[0] == n, ("values", tuple(values.shape), n)
        v = values.detach().contiguous()
        keep = [v, moments]
        a = self._walk_args(_capi.DistortionArgs, rcpt, tile_rows, profile)
        a.power, a.values, a.moments = int(power), v.data_ptr(), moments.data_ptr()
        if out is not None:
            a.out = out.data_ptr()
            keep.append(out)
        if dL_dout is not None:
            g = dL_dout.to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(g.shape) == (self.height, self.width), ("dL_ddistortion_map", tuple(g.shape))
            self._check_into(into, (n,))
            res = into if into is not None else torch.empty((n,), dtype=torch.float32, device=dev)
            self._bw.fit(n)
            a.dL_dout, a.dL_dvalues = g.data_ptr(), res.data_ptr()
            a.value_sums_f64 = self._bw.sums("distortion_sums_f64", n).data_ptr()
            keep += [g, res]
        return a, keep

    def render_distortion(self, values: torch.Tensor, *, power: int = 2, receipt: "_capi.ForwardReceipt | None" = None,
                          tile_rows: "tuple[int, int] | None" = None, into: "torch.Tensor | None" = None, profile: bool = False,
                          sync: bool = True) -> torch.Tensor:
        """[H,W]: the distortion map sum_i sum_j w_i w_j |m_i - m_j|^power of the last draw() (gsr_distortion_forward), w = alpha T
        with that call's own alpha, T and decisions — call it after a draw() and before the next one. values: float32 [N] on this
        device, one scalar m per Gaussian (view depth, inverse depth, ...). power: 2, or 1 — signed in list order, which is the
        absolute form wherever the values do not decrease along the lists (the frame's view depth). receipt: default this
        object's last draw(). tile_rows: the band to write, which must be that of the draw(); other rows are left alone. into: a
        float32 [H,W] tensor on this device, contiguous, written and returned; else a new tensor, zeros outside the band.
        The per-pixel moments [3,H,W] the gradient needs are kept by this object (a new tensor per call), keyed to the receipt's
        serial and the power: distortion_backward / backward(distortion=...) of another frame or power are refused.
        One more walk over the sorted lists (refused after draw(sorted_lists=False)). profile: last_distortion_ms gets the time."""
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "render_distortion needs the receipt of a draw()"
        assert power in (1, 2), ("power", power)
        shape = (self.height, self.width)
        self._check_into(into, shape)
        out = into if into is not None else self._new_output(rcpt, tile_rows, shape)
        moments = self._new_output(rcpt, tile_rows, (3,) + shape)
        a, _keep = self._distortion_call(rcpt, values, power, moments, out=out, tile_rows=tile_rows, profile=profile)
        self._distortion_moments = (None, 0, None)
        self._call("gsr_distortion_forward", a, ms="last_distortion_ms")
        self._distortion_moments = (int(rcpt.serial), int(power), moments)
        if sync:
            torch.cuda.current_stream(self.device).synchronize()
        return out

    def distortion_backward(self, values: torch.Tensor, dL_dmap: torch.Tensor, *, power: int = 2,
                            receipt: "_capi.ForwardReceipt | None" = None, tile_rows: "tuple[int, int] | None" = None,
                            into: "torch.Tensor | None" = None, moments: "torch.Tensor | None" = None, profile: bool = False,
                            sync: bool = True) -> torch.Tensor:
        """dL_dvalues [N] of sum(dL_dmap * render_distortion(values, power=power)) for the last draw() (gsr_distortion_backward
        with no geometry sums: the frozen-geometry case — nothing else is computed and no scratch shared with backward() is
        touched; for the geometry's gradients too, pass distortion= to backward()). dL_dmap: [H,W]. moments: the [3,H,W] tensor
        of that render_distortion call (default: the one this object kept, refused when it is of another frame or power).
        The scratch (8 N bytes of doubles) is kept by this object, zero between calls and dropped if a call fails. into: a
        float32 [N] tensor on this device, contiguous, written in full and returned."""
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "distortion_backward needs the receipt of a draw()"
        assert power in (1, 2), ("power", power)
        a, keep = self._distortion_call(rcpt, values, power, self._distortion_moments_of(rcpt, power, moments), dL_dout=dL_dmap,
                                        into=into, tile_rows=tile_rows, profile=profile)
        self._call("gsr_distortion_backward", a, drop=("distortion_sums_f64",), ms="last_distortion_ms", sync=sync)
        return keep[-1]

    # -- the median depth map and the per-pixel Gaussian ids (include/gsrast_amd_median.h) ----
    def render_median(self, values: "torch.Tensor | None" = None, *, threshold: float = 0.5, ids: bool = True, dominant: bool = False,
                      receipt: "_capi.ForwardReceipt | None" = None, tile_rows: "tuple[int, int] | None" = None,
                      out: "dict | None" = None, profile: bool = False, sync: bool = True) -> dict:
        """The median map and the per-pixel Gaussian ids of the last draw() (gsr_median_forward), with that call's own alpha, T and
        decisions — call it after a draw() and before the next one. Returns a dict of new tensors:
          "map" [H,W] float32 (with `values`: float32 [N] on this device, one scalar per Gaussian — the view depth for the median
              depth): values[i] of the record i the pixel selected, the value's own bits; 0 where nothing was blended;
          "ids" [H,W] int32 (ids=True): that record's Gaussian, the last blended record with a transmittance above `threshold` in
              front of it; -1 (GSR_MEDIAN_NONE) where nothing was blended. threshold: 0.5 the median of 2DGS, 0 the last blended
              record, just under 1 (np.nextafter(1, 0)) the first; 0 <= threshold < 1;
          "dominant_ids" [H,W] int32 (dominant=True): the Gaussian with the largest blending weight alpha T of the pixel
              (ContributionStats' `dominant` decision, per pixel); -1 where nothing was blended.
        At least one of the three must be asked for. The map is a STEP function of the geometry: only `values` receives a gradient
        (median_backward). receipt: default this object's last draw(). tile_rows: the band to walk and write, any band inside the
        rows of the draw() (default: those rows); other rows are left alone. out: {"map" / "ids" / "dominant_ids": tensor} of the
        caller's, contiguous on this device, float32 / int32 [H,W], written instead of new ones (which are 0 / -1 outside the band).
        One more walk over the sorted lists (refused after draw(sorted_lists=False)). profile: last_median_ms gets the time."""
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "render_median needs the receipt of a draw()"
        dev, shape = self.device, (self.height, self.width)
        want = (("map",) if values is not None else ()) + (("ids",) if ids else ()) + (("dominant_ids",) if dominant else ())
        assert want, "render_median: nothing asked for (values, ids or dominant)"
        out = dict(out or {})
        assert set(out) <= set(want), ("out", sorted(out), want)
        res = {}
        for k in want:
            dtype = torch.float32 if k == "map" else torch.int32
            t = out.get(k)
            if t is None:
                t = (torch.zeros(shape, dtype=dtype, device=dev) if k == "map" else torch.full(shape, -1, dtype=dtype, device=dev))
            assert t.dtype == dtype and t.device == dev and t.is_contiguous() and tuple(t.shape) == shape, (k, t.dtype, tuple(t.shape))
            res[k] = t
        a = self._walk_args(_capi.MedianArgs, rcpt, tile_rows, profile)
        a.threshold = float(threshold)
        keep = None
        if values is not None:
            assert isinstance(values, torch.Tensor) and values.dtype == torch.float32 and values.device == dev, "values: a float32 tensor on this device"
            assert values.dim() == 1 and values.shape[0] == self.num_gaussians, ("values", tuple(values.shape), self.num_gaussians)
            keep = values.detach().contiguous()
            a.values, a.out = keep.data_ptr(), res["map"].data_ptr()
        if ids:
            a.ids = res["ids"].data_ptr()
        if dominant:
            a.dominant_ids = res["dominant_ids"].data_ptr()
        self._call("gsr_median_forward", a, ms="last_median_ms", sync=sync)
        return res

    def median_backward(self, ids: torch.Tensor, dL_dmap: torch.Tensor, *, tile_rows: "tuple[int, int] | None" = None,
                        into: "torch.Tensor | None" = None, profile: bool = False, sync: bool = True) -> torch.Tensor:
        """dL_dvalues [N] of sum(dL_dmap * render_median(values)["map"]) with the selection held fixed (gsr_median_backward):
        row i is the sum of dL_dmap over the pixels whose id is i. ids: the int32 [H,W] "ids" of that render_median call; dL_dmap:
        [H,W]. The call reads nothing of the frame: it is valid after this object has drawn again. tile_rows: the band of that
        call (default: every row). The scratch (8 N bytes of doubles) is kept by this object, zero between calls and dropped if
        a call fails. into: a float32 [N] tensor on this device, contiguous, written in full and returned."""
        n, dev = self.num_gaussians, self.device
        assert isinstance(ids, torch.Tensor) and ids.dtype == torch.int32 and ids.device == dev and ids.is_contiguous(), "ids: the int32 map of render_median"
        assert tuple(ids.shape) == (self.height, self.width), ("ids", tuple(ids.shape))
        g = dL_dmap.to(device=dev, dtype=torch.float32).contiguous()
        assert tuple(g.shape) == (self.height, self.width), ("dL_dmap", tuple(g.shape))
        self._check_into(into, (n,))
        res = into if into is not None else torch.empty((n,), dtype=torch.float32, device=dev)
        self._bw.fit(n)
        a = _capi.MedianArgs()
        a.struct_size = C.sizeof(_capi.MedianArgs)
        a.flags = _capi.GSR_FLAG_PROFILE if profile else 0
        a.num_gaussians, a.width, a.height = n, self.width, self.height
        a.ids, a.dL_dout, a.dL_dvalues = ids.data_ptr(), g.data_ptr(), res.data_ptr()
        a.value_sums_f64 = self._bw.sums("median_sums_f64", n).data_ptr()
        if tile_rows is not None:
            a.tile_row_begin, a.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        a.stream = _capi.stream(dev)
        self._call("gsr_median_backward", a, drop=("median_sums_f64",), ms="last_median_ms", sync=sync)
        return res

    def pick(self, x: int, y: int, *, threshold: float = 0.5, dominant: bool = False) -> "int | None":
        """Which Gaussian is under pixel (x, y) of the last draw(): the index render_median's "ids" (dominant=True: "dominant_ids")
        has there, or None where nothing was blended. Walks only the tile row that holds y; one synchronisation."""
        x, y = int(x), int(y)
        assert 0 <= x < self.width and 0 <= y < self.height, ("pick", x, y)
        rcpt = self.last_receipt
        assert rcpt is not None, "pick needs a draw()"
        row = y // 16
        if not (int(rcpt.tile_row_begin) <= row < int(rcpt.tile_row_end)):
            return None                          # (the draw() did not cover this row)
        res = self.render_median(threshold=threshold, ids=not dominant, dominant=dominant, tile_rows=(row, row + 1), sync=False)
        i = int(res["dominant_ids" if dominant else "ids"][y, x])
        return None if i < 0 else i

    def absgrad(self, dL_dout: torch.Tensor, *, dL_ddepth: "torch.Tensor | None" = None, depth: "bool | str | None" = None,
                dL_dalpha: "torch.Tensor | None" = None, receipt: "_capi.ForwardReceipt | None" = None, semantics: str = "gscuda",
                tile_rows: "tuple[int, int] | None" = None, into: "torch.Tensor | None" = None, sync: bool = True,
                profile: bool = False) -> torch.Tensor:
        """The absolute screen-space gradient of the last draw() (AbsGS; gsr_absgrad of include/gsrast_amd_absgrad.h): [N,2],
        per Gaussian and axis the sum over pixels of |each pixel's share of dL_dmean2D| — where backward()'s dL_dmean2D is the
        absolute value of the sum at best. dL_dout, dL_ddepth, depth, dL_dalpha, receipt (a receipt is required: default this
        object's last draw()), semantics and tile_rows as backward() takes them, and for the same frame: the result is that of
        the loss backward() differentiates with the same arguments, its three terms joined per pixel before the absolute value
        is taken. Pixel units, no NDC factor, as dL_dmean2D: densify.DensityStats.update(absgrad=True) takes it.
        One more walk over the sorted lists (refused after draw(sorted_lists=False)); nothing of the forward state is written,
        and backward() may run before or after it. The scratch (16 N bytes of doubles) is kept by this object, zero between
        calls and dropped if a call fails. into: a float32 [N,2] tensor on this device, contiguous, written in full and
        returned; else a new tensor. profile: last_absgrad_ms gets the pass's time."""
        n, dev = self.num_gaussians, self.device
        rcpt = self.last_receipt if receipt is None else receipt
        assert rcpt is not None, "absgrad needs the receipt of a draw()"
        assert semantics in ("gscuda", "inria"), semantics
        self._check_dL_dalpha(dL_dalpha)
        g = dL_dout.to(device=dev, dtype=torch.float32).contiguous()
        assert g.shape == (3, self.height, self.width)
        self._check_into(into, (n, 2))
        gd, mode = self._depth_gradient(dL_ddepth, depth)
        self._bw.fit(n)
        b = self._backward_args(rcpt, self._colors_of(rcpt), semantics, 3)
        b.dL_dout_color = g.data_ptr()
        if dL_ddepth is not None:
            b.dL_dout_depth = gd.data_ptr()
        if tile_rows is not None:
            b.tile_row_begin, b.tile_row_end = int(tile_rows[0]), int(tile_rows[1])
        out = into if into is not None else torch.empty((n, 2), dtype=torch.float32, device=dev)
        a = _capi.AbsgradArgs()
        a.struct_size = C.sizeof(_capi.AbsgradArgs)
        a.flags = (_capi.GSR_FLAG_PROFILE if profile else 0) | (_capi.GSR_FLAG_DEPTH_INVERSE if mode == "inverse" else 0)
        a.backward = C.pointer(b)
        ga = dL_dalpha.contiguous() if dL_dalpha is not None else None
        a.dL_dout_alpha = ga.data_ptr() if ga is not None else None
        a.abs_dL_dmean2D = out.data_ptr()
        a.sums_f64 = self._bw.sums("absgrad_sums_f64", n, 2).data_ptr()
        self._call("gsr_absgrad", a, drop=("absgrad_sums_f64",), ms="last_absgrad_ms", sync=sync)
        return out

    def _colors_of(self, rcpt: "_capi.ForwardReceipt | None") -> "torch.Tensor | None":
        """The precomputed colours the draw() of `rcpt` composited, None where it took its geomState.rgb: they are recorded
        with the call's serial, so a receipt of another call gets None (that call's colours are its geomState.rgb)."""
        serial, col = self._colors_of_call
        return col if rcpt is None or int(rcpt.serial) == serial else None

    def camera_backward(self, grads: dict, *, semantics: str = "gscuda", sh_degree: int = 3, depth: "bool | str | None" = None,
                        shs_colour: "bool | None" = None, receipt: "_capi.ForwardReceipt | None" = None,
                        profile: bool = False, sync: bool = True, into: "torch.Tensor | None" = None) -> dict:
        """gsr_camera_backward alone, on the current stream: the gradients w.r.t. the camera of the last draw(), from the
        per-Gaussian gradients its gsr_backward returned — grads["dL_dmean2D"] [N,2], grads["dL_dcov2D"] [N,4], with a depth
        gradient grads["dL_ddepths"] [N] (depth: the channel's mode, True or "inverse"), and grads["dL_dcolors"] [N,3] when
        the colours came from SH under semantics="inria" (shs_colour; default: from the draw() whose receipt is given — this
        object's last draw() without one — as backward() decides it: colours from SH unless that draw took colors_precomp).
        Returns float32 device tensors dL_dview_matrix (16,), dL_dproj_matrix (16,), dL_dcam_pos (3,) in the layouts of
        Camera.view / .proj / .cam_pos, owned by this object and overwritten by the next call. The scratch
        (gsr_camera_backward_scratch_bytes) is kept by this object. backward(camera=True) calls this.
        into: a (35,) float32 tensor on this device, view | proj | cam_pos — the result is written there and returned as
        views of it, and this object's own gradient buffer is left alone."""
        assert semantics in ("gscuda", "inria") and depth in (None, False, True, "inverse"), (semantics, depth)
        n, dev = self.num_gaussians, self.device
        inria = semantics == "inria"
        if shs_colour is None:
            shs_colour = inria and self._colors_of(self.last_receipt if receipt is None else receipt) is None
        gst = _capi.GeometryState()
        self.lib.gsr_geometry_from_chunk(self.geom.base(), n, C.byref(gst))
        self._bw.fit(n)
        scratch = self._bw.get("camera_scratch", int(self.lib.gsr_camera_backward_scratch_bytes(n)), dtype=torch.uint8)
        g = self._bw.get("camera_grad", 35)

        def ptr(k):
            t = grads[k]
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == dev and t.shape[0] == n, k
            return t.data_ptr()
        a = _capi.CameraBackwardArgs()
        a.struct_size = C.sizeof(_capi.CameraBackwardArgs)
        a.flags = ((_capi.GSR_FLAG_PROFILE if profile else 0) | (_capi.GSR_FLAG_SEMANTICS_INRIA if inria else 0)
                   | (_capi.GSR_FLAG_DEPTH_INVERSE if depth == "inverse" else 0))
        a.num_gaussians, a.width, a.height = n, self.width, self.height
        a.means3D, a.view_matrix, a.proj_matrix = self.means3D.data_ptr(), self._view.data_ptr(), self._proj.data_ptr()
        a.cam_pos = self._cam_pos.data_ptr()
        a.tan_fovx, a.tan_fovy = self._tan
        a.cov3D, a.radii = gst.cov3D, gst.internal_radii
        if shs_colour:
            a.shs, a.clamped, a.sh_dims = self.shs.data_ptr(), gst.clamped, int(sh_degree)
            a.dL_dcolors = ptr("dL_dcolors")
        a.dL_dmean2D, a.dL_dcov2D = ptr("dL_dmean2D"), ptr("dL_dcov2D")
        if depth:
            a.dL_ddepths = ptr("dL_ddepths")
        if into is not None:
            self._check_into(into, (35,))
            g = into
        a.dL_dview_matrix, a.dL_dproj_matrix, a.dL_dcam_pos = g[0:16].data_ptr(), g[16:32].data_ptr(), g[32:35].data_ptr()
        a.scratch = scratch.data_ptr()
        a.stream = _capi.stream(dev)
        self._call("gsr_camera_backward", a, ms="last_camera_ms", sync=sync)
        return {"dL_dview_matrix": g[0:16], "dL_dproj_matrix": g[16:32], "dL_dcam_pos": g[32:35]}

    # -- state inspection (what the reference's Inspector does through fromChunk) ------
    def map_geometry_state(self) -> dict:
        st = _capi.GeometryState()
        self.lib.gsr_geometry_from_chunk(self.geom.base(), self.num_gaussians, C.byref(st))
        n, v = self.num_gaussians, self.geom.view
        return {
            "tilesTouched": v(st.tiles_touched, n, torch.int32),
            "depths": v(st.depths, n, torch.float32),
            "radii": v(st.internal_radii, n, torch.int32),
            "means2D": v(st.means2D, 2 * n, torch.float32).view(n, 2),
            "cov3D": v(st.cov3D, 6 * n, torch.float32).view(n, 6),
            "conicOpacity": v(st.conic_opacity, 4 * n, torch.float32).view(n, 4),
            "rgb": v(st.rgb, 3 * n, torch.float32).view(n, 3),
            "pointOffsets": v(st.point_offsets, n, torch.int32),
            # bool[3 N]: colour channel clamped at zero (written under semantics="inria" with SH colours only)
            "clamped": v(st.clamped, 3 * n, torch.uint8).view(torch.bool).view(n, 3),
        }

    def map_image_state(self) -> dict:
        st = _capi.ImageState()
        P = self.width * self.height
        self.lib.gsr_image_from_chunk(self.image.base(), P, C.byref(st))
        T = ((self.width + 15) // 16) * ((self.height + 15) // 16)
        v = self.image.view
        return {
            "ranges": v(st.ranges, 2 * T, torch.int32).view(T, 2),
            "nContrib": v(st.n_contrib, P, torch.int32).view(self.height, self.width),
            "finalT": v(st.accum_alpha, P, torch.float32).view(self.height, self.width),
        }

    def map_binning_state(self) -> dict:
        st = _capi.BinningState()
        R = self.last_num_rendered
        self.lib.gsr_binning_from_chunk(self.binning.base(), R, C.byref(st))
        v = self.binning.view
        return {
            "keys_unsorted": v(st.keys_unsorted, R, torch.int64),
            "keys": v(st.keys, R, torch.int64),
            "values_unsorted": v(st.values_unsorted, R, torch.int32),
            "values": v(st.values, R, torch.int32),
        }


# ---- stage-level wrappers (unit parity tests) ------------------------------------------
def inclusive_scan_u32(x: torch.Tensor) -> torch.Tensor:
    assert x.dtype == torch.int32 and x.is_cuda and x.is_contiguous()
    out = torch.empty_like(x)
    temp = torch.empty(max(int(_capi.lib().gsr_scan_temp_bytes(x.numel())), 128), dtype=torch.uint8, device=x.device)
    _capi.call("gsr_inclusive_scan_u32", x.data_ptr(), out.data_ptr(), x.numel(), temp.data_ptr(), _capi.stream(x.device), device=x.device)
    torch.cuda.current_stream(x.device).synchronize()
    return out


def sort_pairs(keys: torch.Tensor, values: torch.Tensor, end_bit: int = 64, begin_bit: int = 0, sync: bool = True,
               out=None, temp=None):
    assert keys.dtype == torch.int64 and values.dtype == torch.int32 and keys.is_cuda
    assert keys.is_contiguous() and values.is_contiguous() and keys.numel() == values.numel()
    n = keys.numel()
    ko, vo = out if out is not None else (torch.empty_like(keys), torch.empty_like(values))
    if temp is None:
        temp = torch.empty(max(int(_capi.lib().gsr_sort_temp_bytes(n)), 128), dtype=torch.uint8, device=keys.device)
    _capi.call("gsr_sort_pairs_u64_u32", keys.data_ptr(), ko.data_ptr(), values.data_ptr(), vo.data_ptr(), n, begin_bit, end_bit,
               temp.data_ptr(), _capi.stream(keys.device), device=keys.device)
    if sync:
        torch.cuda.current_stream(keys.device).synchronize()
    return ko, vo
