"""ctypes front end of the reference itself, compiled for the host (oracle/_ref/libgscuda_ref.so: the reference's own
GSCuda.cu / AuxBuffer.cu / CudaHelpers.cu against the stand-ins of oracle/ref_host/, built by oracle/build_ref.py).

TEST INFRASTRUCTURE: importable from tests/ only. Shaped like cpu_oracle.forward: the same scene / camera arguments,
the same keys in the returned dict — except records_staged, which the reference does not count.

What a comparison against this library pins is the reference's text. It does not pin: float -> int conversions that
leave the range of int or start from NaN (undefined on the host, saturating on the device), nvcc's contraction of
multiply-adds, CUDA's expf (this build calls the host libm's), and glm's operation orders (restated in the stand-in).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build_ref

_lib = None


class ForwardArgs(C.Structure):
    _fields_ = [
        ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("scale_modifier", C.c_float), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
        ("background", C.c_void_p), ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("cov3d_precomp", C.c_void_p),
        ("view", C.c_void_p), ("proj", C.c_void_p), ("cam_pos", C.c_void_p),
        ("out_color", C.c_void_p), ("radii", C.c_void_p), ("rects", C.c_void_p),
        ("tiles_touched", C.c_void_p), ("depths", C.c_void_p), ("clamped", C.c_void_p), ("internal_radii", C.c_void_p),
        ("means2D", C.c_void_p), ("cov3D", C.c_void_p), ("conic_opacity", C.c_void_p), ("rgb", C.c_void_p),
        ("point_offsets", C.c_void_p),
        ("ranges", C.c_void_p), ("n_contrib", C.c_void_p), ("accum_alpha", C.c_void_p),
        ("num_rendered", C.c_uint32),
        ("geometry_calls", C.c_int32), ("image_calls", C.c_int32), ("binning_calls", C.c_int32),
        ("geometry_bytes", C.c_uint64), ("image_bytes", C.c_uint64), ("binning_bytes", C.c_uint64),
    ]


def available() -> bool:
    """The library exists or can be built (the reference tree is present)."""
    return os.path.exists(build_ref.LIB_PATH) or build_ref.reference_present()


def lib() -> C.CDLL:
    """Builds the library on first use when the reference tree is there (as cpu_oracle.lib() builds the oracle)."""
    global _lib
    if _lib is None:
        path = build_ref.build()
        if path is None:
            raise RuntimeError("oracle/_ref/libgscuda_ref.so is missing and there is no reference tree to build it from "
                               f"({build_ref.source_dir()}); set GSR_REFERENCE_DIR")
        L = C.CDLL(path)
        L.gsref_higher_msb.restype = C.c_uint32
        L.gsref_higher_msb.argtypes = [C.c_uint32]
        for name in ("geometry", "image", "binning", "points_geometry", "points_image"):
            fn = getattr(L, "gsref_required_" + name)
            fn.restype, fn.argtypes = C.c_size_t, [C.c_int]
        for name in ("geometry", "image", "binning", "points_image"):
            fn = getattr(L, f"gsref_{name}_from_chunk")
            fn.restype, fn.argtypes = None, [C.c_uint64, C.c_int, C.POINTER(C.c_uint64)]
        L.gsref_set_temp_sizes.restype, L.gsref_set_temp_sizes.argtypes = None, [C.c_size_t, C.c_size_t]
        L.gsref_forward.restype, L.gsref_forward.argtypes = C.c_int, [C.POINTER(ForwardArgs)]
        L.gsref_forward_points.restype = C.c_int
        L.gsref_last_lists.restype, L.gsref_last_lists.argtypes = C.c_uint64, [C.c_void_p] * 4
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def higher_msb(n: int) -> int:
    return int(lib().gsref_higher_msb(n))


def set_temp_sizes(scan_bytes: int = 1, sort_bytes: int = 1) -> None:
    """The sizes the cub stand-in reports for its scan / sort temporaries from now on (defaults: the stand-in's own 1 byte).
    CUB's sizes are a property of CUB, not of the reference: a test that compares chunk layouts sets them to the sizes the
    library under test uses, so that every offset can be compared."""
    lib().gsref_set_temp_sizes(scan_bytes, sort_bytes)


GEOMETRY_FIELDS = ("tilesTouched", "scanSize", "scanningSpace", "depths", "clamped", "internalRadii", "means2D", "cov3D",
                   "conicOpacity", "rgb", "pointOffsets", "end")
IMAGE_FIELDS = ("ranges", "nContrib", "accumAlpha", "end")
BINNING_FIELDS = ("pointListKeysUnsorted", "pointListKeys", "pointListUnsorted", "pointList", "sortingSize", "listSortingSpace", "end")
POINTS_IMAGE_FIELDS = ("depth", "outColor", "defaultDepth", "end")


def from_chunk(which: str, base: int, n: int) -> dict:
    """The reference's own fromChunk of gs::GeometryState / gs::ImageState / gs::BinningState / pc::ImageState
    (which = geometry | image | binning | points_image) on a chunk at address `base`: every pointer as an integer, the
    sizes it took from the scan / sort, and the chunk's end."""
    fields = {"geometry": GEOMETRY_FIELDS, "image": IMAGE_FIELDS, "binning": BINNING_FIELDS, "points_image": POINTS_IMAGE_FIELDS}[which]
    out = (C.c_uint64 * len(fields))()
    getattr(lib(), f"gsref_{which}_from_chunk")(base, n, out)
    return dict(zip(fields, (int(v) for v in out)))


def required(which: str, n: int) -> int:
    return int(getattr(lib(), "gsref_required_" + which)(n))


def forward(scene: dict, cam, background=(0.0, 0.0, 0.0), use_rects: bool = True, scale_modifier: float = 1.0,
            out_init: np.ndarray | None = None, colors_precomp: np.ndarray | None = None,
            cov3d_precomp: np.ndarray | None = None, callers_radii: bool = True) -> dict:
    """gscuda::forward (GSCuda.cu:695-811) on the CPU; every array of the three states, the caller's rects / radii and
    the image. callers_radii=False passes radii = nullptr: the reference then uses GeometryState::internalRadii (returned
    as "radii" too). Arrays the reference leaves unwritten are zero (the chunks start zero-filled)."""
    L = lib()
    n = int(scene["means3D"].shape[0])
    W, H = int(cam.width), int(cam.height)
    P = W * H
    gx, gy = (W + 15) // 16, (H + 15) // 16
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    keep = [f32(scene[k]) for k in ("means3D", "shs", "opacities", "scales", "rotations")]
    assert keep[0].shape == (n, 4) and keep[3].shape == (n, 4) and keep[4].shape == (n, 4) and keep[1].shape == (n, 48)
    view, proj, pos, bg = f32(cam.view), f32(cam.proj), f32(cam.cam_pos), f32(np.asarray(background))
    colors = None if colors_precomp is None else f32(colors_precomp)
    cov3d_in = None if cov3d_precomp is None else f32(cov3d_precomp)
    o = {
        "radii": np.zeros(n, np.int32), "internalRadii": np.zeros(n, np.int32), "means2D": np.zeros((n, 2), np.float32),
        "depths": np.zeros(n, np.float32), "cov3D": np.zeros((n, 6), np.float32), "rgb": np.zeros((n, 3), np.float32),
        "conicOpacity": np.zeros((n, 4), np.float32), "tilesTouched": np.zeros(n, np.uint32),
        "pointOffsets": np.zeros(n, np.uint32), "clamped": np.zeros((n, 3), np.uint8),
        "rects": np.zeros((n, 2), np.int32) if use_rects else None,
        "out_color": np.zeros((3, H, W), np.float32) if out_init is None else f32(out_init).copy(),
        "finalT": np.zeros((H, W), np.float32), "nContrib": np.zeros((H, W), np.uint32),
    }
    ranges_px = np.zeros((P, 2), np.uint32)
    a = ForwardArgs()
    a.num_gaussians, a.width, a.height = n, W, H
    a.scale_modifier, a.tan_fovx, a.tan_fovy = scale_modifier, cam.tan_fovx, cam.tan_fovy
    a.background, a.means3D, a.shs, a.opacities, a.scales, a.rotations = (_p(v) for v in (bg, keep[0], keep[1], keep[2], keep[3], keep[4]))
    a.colors_precomp, a.cov3d_precomp = _p(colors), _p(cov3d_in)
    a.view, a.proj, a.cam_pos = _p(view), _p(proj), _p(pos)
    a.out_color, a.radii, a.rects = _p(o["out_color"]), (_p(o["radii"]) if callers_radii else None), _p(o["rects"])
    a.tiles_touched, a.depths, a.clamped, a.internal_radii = _p(o["tilesTouched"]), _p(o["depths"]), _p(o["clamped"]), _p(o["internalRadii"])
    a.means2D, a.cov3D, a.conic_opacity, a.rgb, a.point_offsets = (_p(o[k]) for k in ("means2D", "cov3D", "conicOpacity", "rgb", "pointOffsets"))
    a.ranges, a.n_contrib, a.accum_alpha = _p(ranges_px), _p(o["nContrib"]), _p(o["finalT"])
    rc = L.gsref_forward(C.byref(a))
    assert rc == 0, rc
    R = int(a.num_rendered)
    lists = {"keys_unsorted": np.zeros(R, np.uint64), "keys": np.zeros(R, np.uint64),
             "values_unsorted": np.zeros(R, np.uint32), "values": np.zeros(R, np.uint32)}
    if R > 0:
        got = L.gsref_last_lists(*(_p(lists[k]) for k in ("keys_unsorted", "keys", "values_unsorted", "values")))
        assert got == R, (got, R)
    else:
        assert L.gsref_last_lists(None, None, None, None) == 0
    if not callers_radii:
        o["radii"] = o["internalRadii"].copy()
    o.update(lists)
    assert not ranges_px[gx * gy:].any(), "ranges beyond the tile grid were written"
    o["ranges"] = ranges_px[: gx * gy].copy()
    o["num_rendered"] = R
    o["alloc_calls"] = (int(a.geometry_calls), int(a.image_calls), int(a.binning_calls))
    o["alloc_bytes"] = (int(a.geometry_bytes), int(a.image_bytes), int(a.binning_bytes))
    return o


def forward_points(means3, shs, proj, width, height, background):
    """gscuda::forwardPoints (GSCuda.cu:102-155) on the CPU: (out_color [3,H,W], depth [H,W]), shaped like
    points_np.forward_points. The host build runs the threads in index order, so where several points land on one pixel
    the nearest wins and, among equal depths, the lowest index: the outcome points_np states."""
    L = lib()
    m = np.ascontiguousarray(np.asarray(means3, np.float32)[:, :3])
    sh = np.ascontiguousarray(shs, np.float32)
    pr = np.ascontiguousarray(proj, np.float32)
    bg = np.ascontiguousarray(np.asarray(background), np.float32)
    out = np.zeros((3, height, width), np.float32)
    depth = np.zeros((height, width), np.float32)
    calls, nbytes = (C.c_int32 * 3)(), (C.c_uint64 * 3)()
    rc = L.gsref_forward_points(C.c_int(m.shape[0]), C.c_int(width), C.c_int(height), _p(bg), _p(m), _p(sh), _p(pr), _p(out), _p(depth),
                                calls, nbytes)
    assert rc == 0, rc
    forward_points.last_alloc = (tuple(calls), tuple(int(b) for b in nbytes))
    return out, depth
