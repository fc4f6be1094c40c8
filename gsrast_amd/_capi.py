"""ctypes binding of include/gsrast_amd.h, include/gsrast_amd_init.h, include/gsrast_amd_opacity.h, include/gsrast_amd_mcmc.h,
include/gsrast_amd_contrib.h, include/gsrast_amd_antialias.h, include/gsrast_amd_filter3d.h, include/gsrast_amd_absgrad.h,
include/gsrast_amd_features.h, include/gsrast_amd_distortion.h, include/gsrast_amd_normals.h and include/gsrast_amd_median.h (the C
ABI of libgsrast_amd.so).

There is no fallback: if the HIP library has not been built, importing the product path
raises. Field order and types below mirror the header exactly.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# GSR_LIB_TAG selects a tuning build made with `python -m gsrast_amd.build --tag NAME` (experiments only).
_TAG = os.environ.get("GSR_LIB_TAG", "")
LIB_PATH = os.path.join(_HERE, "lib", f"libgsrast_amd{'_' + _TAG if _TAG else ''}.so")

GSR_OK = 0
GSR_ERR_INVALID_ARG = 1
GSR_ERR_ALLOC = 2
GSR_ERR_HIP = 3
GSR_ERR_NO_DEVICE = 4
GSR_ERR_TOO_LARGE = 5
GSR_ERR_INTERNAL = 6
GSR_ERR_STALE_RECEIPT = 7

GSR_FLAG_PROFILE = 0x1
GSR_FLAG_COUNT_STAGED = 0x2
GSR_FLAG_SEMANTICS_INRIA = 0x4
GSR_FLAG_PLAN_SORT = 0x8
GSR_FLAG_PLAN_BLOCKS = 0x10
GSR_FLAG_OVERLAP_EMIT = 0x20
GSR_FLAG_NO_SORTED_LISTS = 0x40
GSR_FLAG_NO_TILE_HISTORY = 0x80
GSR_FLAG_SERIAL_EMIT = 0x100
GSR_FLAG_NO_DEEP_TILES = 0x200
GSR_FLAG_DEEP_TILES_ALL = 0x400
GSR_FLAG_DEEP_WAVES_8 = 0x800
GSR_FLAG_DEEP_WAVES_16 = 0x1000
GSR_FLAG_DEPTH_INVERSE = 0x2000
GSR_PLAN_LISTS_SKIPPED = 0x100
GSR_PLAN_BLEND_FROM_LISTS = 0x200
GSR_PLAN_TILES_REORDERED = 0x400
GSR_PLAN_EMIT_OVERLAPPED = 0x800
GSR_PLAN_COLORS_BESIDE = 0x1000
GSR_PLAN_TILE_ORDER_DROPPED = 0x2000
GSR_PLAN_DEEP_TILES = 0x4000
GSR_SH_LAYOUT_FILE, GSR_SH_LAYOUT_COEFFICIENT_MAJOR = 0, 1
PLAN_NAMES = {0: "none", 1: "sort", 2: "blocks", 3: "generic"}
GSR_NUM_STAGES = 8
STAGE_NAMES = ("preprocess", "scan", "depth_order", "duplicate", "sort_pass1", "sort_pass2", "ranges", "blend")

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class GeometryState(C.Structure):
    _fields_ = [("tiles_touched", C.c_void_p), ("scan_size", C.c_size_t), ("num_rendered", C.c_uint32),
                ("scanning_space", C.c_void_p), ("depths", C.c_void_p), ("clamped", C.c_void_p),
                ("internal_radii", C.c_void_p), ("means2D", C.c_void_p), ("cov3D", C.c_void_p),
                ("conic_opacity", C.c_void_p), ("rgb", C.c_void_p), ("point_offsets", C.c_void_p)]


class ImageState(C.Structure):
    _fields_ = [("ranges", C.c_void_p), ("n_contrib", C.c_void_p), ("accum_alpha", C.c_void_p)]


class BinningState(C.Structure):
    _fields_ = [("keys_unsorted", C.c_void_p), ("keys", C.c_void_p), ("values_unsorted", C.c_void_p),
                ("values", C.c_void_p), ("sorting_size", C.c_size_t), ("sorting_space", C.c_void_p)]


GSR_RECEIPT_MAGIC = 0x31525347
GSR_LISTS_SKIPPED_STAMP = 0xFFFFFFFF


class ForwardReceipt(C.Structure):
    """gsr_forward_receipt: plain data, copied by value (ctypes copies nested structures on assignment)."""
    _fields_ = [("magic", C.c_uint32), ("plan_used", C.c_uint32),
                ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32),
                ("num_rendered", C.c_uint32), ("num_visible", C.c_uint32), ("serial", C.c_uint32),
                ("geometry_chunk", C.c_void_p), ("image_chunk", C.c_void_p), ("binning_chunk", C.c_void_p),
                ("async_words", C.c_void_p), ("tile_history", C.c_void_p)]

    def copy(self) -> "ForwardReceipt":
        r = ForwardReceipt()
        C.memmove(C.byref(r), C.byref(self), C.sizeof(ForwardReceipt))
        return r


class ForwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("geometry_alloc", ALLOC_FN), ("geometry_user", C.c_void_p),
        ("binning_alloc", ALLOC_FN), ("binning_user", C.c_void_p),
        ("image_alloc", ALLOC_FN), ("image_user", C.c_void_p),
        ("num_gaussians", C.c_int32), ("sh_dims", C.c_int32), ("M", C.c_int32),
        ("background", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32),
        ("means3D", C.c_void_p), ("shs", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("scales", C.c_void_p), ("scale_modifier", C.c_float),
        ("rotations", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("view_matrix", C.c_void_p),
        ("proj_matrix", C.c_void_p), ("cam_pos", C.c_void_p), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
        ("prefiltered", C.c_int32), ("out_color", C.c_void_p), ("radii", C.c_void_p), ("rects", C.c_void_p),
        ("box_min", C.c_void_p), ("box_max", C.c_void_p),
        ("stream", C.c_void_p), ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32),
        ("tile_history", C.c_void_p),
        ("num_rendered", C.c_uint32), ("records_staged", C.c_uint64),
        ("stage_ms", C.c_float * GSR_NUM_STAGES),
        ("plan_used", C.c_uint32),
        ("receipt", ForwardReceipt),
        ("out_depth", C.c_void_p),
    ]


class PointsImageState(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("out_color", C.c_void_p), ("default_depth", C.c_void_p), ("winner", C.c_void_p)]


class BackwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("background", C.c_void_p),
        ("means2D", C.c_void_p), ("conic_opacity", C.c_void_p), ("colors", C.c_void_p), ("cov3D", C.c_void_p),
        ("radii", C.c_void_p), ("ranges", C.c_void_p), ("n_contrib", C.c_void_p), ("final_t", C.c_void_p),
        ("point_list", C.c_void_p),
        ("means3D", C.c_void_p), ("view_matrix", C.c_void_p), ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
        ("dL_dout_color", C.c_void_p),
        ("dL_dmean2D", C.c_void_p), ("dL_dconic_opacity", C.c_void_p), ("dL_dcolors", C.c_void_p),
        ("dL_dcov3D", C.c_void_p), ("dL_dshs", C.c_void_p), ("dL_dcov2D", C.c_void_p),
        ("sums_f64", C.c_void_p),
        ("proj_matrix", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("scale_modifier", C.c_float),
        ("dL_dmeans3D", C.c_void_p), ("dL_dscales", C.c_void_p), ("dL_drotations", C.c_void_p),
        ("stream", C.c_void_p), ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32),
        ("stage_ms", C.c_float * 2),
        ("cam_pos", C.c_void_p), ("shs", C.c_void_p), ("clamped", C.c_void_p), ("sh_dims", C.c_int32),
        ("receipt", ForwardReceipt),
        ("dL_dout_depth", C.c_void_p), ("dL_ddepths", C.c_void_p), ("depth_sums_f64", C.c_void_p),
    ]


class CameraBackwardArgs(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("flags", C.c_uint32),
        ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("means3D", C.c_void_p), ("view_matrix", C.c_void_p), ("proj_matrix", C.c_void_p), ("cam_pos", C.c_void_p),
        ("tan_fovx", C.c_float), ("tan_fovy", C.c_float),
        ("cov3D", C.c_void_p), ("radii", C.c_void_p),
        ("shs", C.c_void_p), ("clamped", C.c_void_p), ("sh_dims", C.c_int32),
        ("dL_dmean2D", C.c_void_p), ("dL_dcov2D", C.c_void_p), ("dL_ddepths", C.c_void_p), ("dL_dcolors", C.c_void_p),
        ("dL_dview_matrix", C.c_void_p), ("dL_dproj_matrix", C.c_void_p), ("dL_dcam_pos", C.c_void_p),
        ("scratch", C.c_void_p), ("stream", C.c_void_p), ("stage_ms", C.c_float),
    ]


GSR_ADAM_MAX_TENSORS = 8


class AdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("row_floats", C.c_int32), ("step_size", C.c_float), ("rs", C.c_float), ("b1c", C.c_float),
                ("b2", C.c_float), ("b2c", C.c_float), ("eps", C.c_float)]


class AdamArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("num_tensors", C.c_int32), ("num_rows", C.c_int64),
                ("visible", C.c_void_p), ("stream", C.c_void_p), ("tensors", AdamTensor * GSR_ADAM_MAX_TENSORS)]


class PhotoLossArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("channels", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("lambda_dssim", C.c_double), ("image", C.c_void_p), ("target", C.c_void_p), ("scratch", C.c_void_p),
                ("out", C.c_void_p), ("dL_dloss", C.c_void_p), ("dL_dimage", C.c_void_p), ("want_backward", C.c_int32),
                ("stream", C.c_void_p)]


class DensifyArray(C.Structure):
    _fields_ = [("src", C.c_void_p), ("src_exp_avg", C.c_void_p), ("src_exp_avg_sq", C.c_void_p),
                ("dst", C.c_void_p), ("dst_exp_avg", C.c_void_p), ("dst_exp_avg_sq", C.c_void_p)]


class DensifyApplyArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("log_shrink", C.c_float), ("n_src", C.c_int64), ("counts", C.c_int32 * 4),
                ("src_of", C.c_void_p), ("noise", C.c_void_p), ("stream", C.c_void_p),
                ("xyz", DensifyArray), ("opacity_logit", DensifyArray), ("log_scale", DensifyArray),
                ("rotation", DensifyArray), ("shs", DensifyArray)]


# name -> (restype, argtypes); this is also the list the symbol test checks against the header.
SIGNATURES = {
    "gsr_geometry_from_chunk": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(GeometryState)]),
    "gsr_image_from_chunk": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(ImageState)]),
    "gsr_binning_from_chunk": (C.c_void_p, [C.c_void_p, C.c_size_t, C.POINTER(BinningState)]),
    "gsr_required_geometry": (C.c_size_t, [C.c_int]),
    "gsr_required_image": (C.c_size_t, [C.c_int]),
    "gsr_required_binning": (C.c_size_t, [C.c_size_t]),
    "gsr_forward": (C.c_int, [C.POINTER(ForwardArgs)]),
    "gsr_backward": (C.c_int, [C.POINTER(BackwardArgs)]),
    "gsr_camera_backward_scratch_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_camera_backward": (C.c_int, [C.POINTER(CameraBackwardArgs)]),
    "gsr_points_image_from_chunk": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(PointsImageState)]),
    "gsr_required_points_image": (C.c_size_t, [C.c_int]),
    "gsr_forward_points": (C.c_int, [C.POINTER(ForwardArgs)]),
    "gsr_last_error": (C.c_int, []),
    "gsr_error_string": (C.c_char_p, [C.c_int]),
    "gsr_last_hip_error": (C.c_char_p, []),
    "gsr_poll_async_error": (C.c_int, [C.POINTER(ForwardReceipt)]),
    "gsr_tile_history_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "gsr_tile_history_destroy": (C.c_int, [C.c_void_p]),
    "gsr_tile_history_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "gsr_tile_history_forget_stream": (C.c_int, [C.c_void_p]),
    "gsr_tile_history_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint32)]),
    "gsr_thread_release": (C.c_int, []),
    "gsr_reread_environment": (None, []),
    "gsr_device_shape": (None, [C.c_int, C.POINTER(C.c_uint32)]),
    "gsr_higher_msb": (C.c_uint32, [C.c_uint32]),
    "gsr_scan_temp_bytes": (C.c_size_t, [C.c_size_t]),
    "gsr_inclusive_scan_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "gsr_sort_temp_bytes": (C.c_size_t, [C.c_size_t]),
    "gsr_sort_pairs_u64_u32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int,
                                         C.c_void_p, C.c_void_p]),
    "gsr_exchange_unique_id": (C.c_int, [C.c_char_p, C.c_char_p]),
    "gsr_exchange_create": (C.c_int, [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "gsr_exchange_bands": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_void_p]),
    "gsr_exchange_plan": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "gsr_exchange_loopback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "gsr_exchange_destroy": (C.c_int, [C.c_void_p]),
    "gsr_exchange_last_error": (C.c_char_p, []),
    "gsr_ply_parse_header": (C.c_int, [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_longlong)]),
    "gsr_ply_activate": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "gsr_colors_from_dc": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_blend_expf": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_footprint_misses_tile": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "gsr_ply_activate_layout": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p]),
    "gsr_activate_params": (C.c_int, [C.c_int] + [C.c_void_p] * 9),
    "gsr_activate_params_backward": (C.c_int, [C.c_int] + [C.c_void_p] * 13),
    "gsr_adam_step": (C.c_int, [C.POINTER(AdamArgs)]),
    "gsr_photo_loss_scratch_bytes": (C.c_size_t, [C.c_int, C.c_int, C.c_int]),
    "gsr_photo_loss_forward": (C.c_int, [C.POINTER(PhotoLossArgs)]),
    "gsr_photo_loss_backward": (C.c_int, [C.POINTER(PhotoLossArgs)]),
    "gsr_densify_accumulate": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "gsr_densify_plan_temp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_densify_plan": (C.c_int, [C.c_int64] + [C.c_void_p] * 5 + [C.c_float] * 5 + [C.c_int32] + [C.c_void_p] * 4),
    "gsr_densify_apply": (C.c_int, [C.POINTER(DensifyApplyArgs)]),
}

# include/gsrast_amd_init.h (initialisation from a point cloud), in the same shape; its own symbol test checks it against that header.
GSR_KNN_LEAF = 64
GSR_KNN_NODE = 32
GSR_KNN_MORTON_BITS = 21
GSR_KNN_MAX_POINTS = 1 << 30
INIT_SIGNATURES = {
    "gsr_knn_temp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_knn_mean_dist2": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# include/gsrast_amd_opacity.h (the accumulated opacity's gradient), in the same shape, with its own symbol test.
OPACITY_SIGNATURES = {
    "gsr_backward_alpha": (C.c_int, [C.POINTER(BackwardArgs), C.c_void_p]),
}

# include/gsrast_amd_mcmc.h (3DGS-MCMC: noise, plan, relocate), in the same shape, with its own symbol test.
GSR_MCMC_MAX_ROWS = (1 << 31) - 1
GSR_MCMC_MAX_RATIO = 51


class McmcNoiseArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("scaler", C.c_float), ("n", C.c_int64), ("xyz", C.c_void_p),
                ("opacity_logit", C.c_void_p), ("log_scale", C.c_void_p), ("rotation", C.c_void_p), ("noise", C.c_void_p),
                ("stream", C.c_void_p)]


class McmcArray(C.Structure):
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p)]


class McmcRelocateArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_opacity", C.c_float), ("n", C.c_int64), ("m", C.c_int64),
                ("sampled", C.c_void_p), ("dst", C.c_void_p),
                ("xyz", McmcArray), ("opacity_logit", McmcArray), ("log_scale", McmcArray), ("rotation", McmcArray), ("shs", McmcArray),
                ("temp", C.c_void_p), ("stream", C.c_void_p)]


MCMC_SIGNATURES = {
    "gsr_mcmc_noise": (C.c_int, [C.POINTER(McmcNoiseArgs)]),
    "gsr_mcmc_plan_temp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_mcmc_plan": (C.c_int, [C.c_int64, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gsr_mcmc_relocate_temp_bytes": (C.c_size_t, [C.c_int64]),
    "gsr_mcmc_relocate": (C.c_int, [C.POINTER(McmcRelocateArgs)]),
}

# include/gsrast_amd_contrib.h (per-Gaussian contribution statistics of a frame), in the same shape, with its own symbol test.
class ContributionArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("means2D", C.c_void_p), ("conic_opacity", C.c_void_p), ("ranges", C.c_void_p), ("n_contrib", C.c_void_p),
                ("point_list", C.c_void_p), ("receipt", ForwardReceipt),
                ("weight_sum", C.c_void_p), ("weight_max", C.c_void_p), ("pixels", C.c_void_p), ("dominant", C.c_void_p),
                ("stream", C.c_void_p), ("stage_ms", C.c_float)]


CONTRIB_SIGNATURES = {
    "gsr_contribution": (C.c_int, [C.POINTER(ContributionArgs)]),
}

# include/gsrast_amd_antialias.h (antialiased splatting: the opacity compensation and its gradient), in the same shape, with its own symbol test.
_ANTIALIAS_COMMON = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                     ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                     ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("scale_modifier", C.c_float),
                     ("means3D", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("opacities", C.c_void_p),
                     ("view_matrix", C.c_void_p), ("proj_matrix", C.c_void_p)]


class AntialiasArgs(C.Structure):
    _fields_ = _ANTIALIAS_COMMON + [("opacities_out", C.c_void_p), ("compensation", C.c_void_p), ("stream", C.c_void_p)]


class AntialiasBackwardArgs(C.Structure):
    _fields_ = _ANTIALIAS_COMMON + [("dL_dopacities_out", C.c_void_p), ("radii", C.c_void_p),
                                    ("dL_dopacities", C.c_void_p), ("dL_dmeans3D", C.c_void_p), ("dL_dscales", C.c_void_p),
                                    ("dL_drotations", C.c_void_p), ("stream", C.c_void_p)]


ANTIALIAS_SIGNATURES = {
    "gsr_antialias_forward": (C.c_int, [C.POINTER(AntialiasArgs)]),
    "gsr_antialias_backward": (C.c_int, [C.POINTER(AntialiasBackwardArgs)]),
}

# include/gsrast_amd_filter3d.h (Mip-Splatting's 3D smoothing filter: sampling rate, smoothing, gradient), in the same shape, with its own symbol test.
GSR_FILTER3D_CAMERA_FLOATS = 20
GSR_FILTER3D_CAMERA_CHUNK = 64


class Filter3dObserveArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("num_gaussians", C.c_int32), ("position_stride", C.c_int32), ("num_cameras", C.c_int32),
                ("positions", C.c_void_p), ("cameras", C.c_void_p), ("min_depth", C.c_void_p), ("stream", C.c_void_p)]


class Filter3dFinalizeArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("num_gaussians", C.c_int32), ("max_focal", C.c_float),
                ("min_depth", C.c_void_p), ("filter", C.c_void_p), ("temp", C.c_void_p), ("temp_bytes", C.c_size_t),
                ("stream", C.c_void_p)]


class Filter3dArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("num_gaussians", C.c_int32),
                ("scales", C.c_void_p), ("opacities", C.c_void_p), ("filter", C.c_void_p),
                ("scales_out", C.c_void_p), ("opacities_out", C.c_void_p), ("stream", C.c_void_p)]


class Filter3dBackwardArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("num_gaussians", C.c_int32),
                ("scales", C.c_void_p), ("opacities", C.c_void_p), ("filter", C.c_void_p),
                ("dL_dscales_out", C.c_void_p), ("dL_dopacities_out", C.c_void_p), ("radii", C.c_void_p),
                ("dL_dscales", C.c_void_p), ("dL_dopacities", C.c_void_p), ("stream", C.c_void_p)]


FILTER3D_SIGNATURES = {
    "gsr_filter3d_temp_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_filter3d_observe": (C.c_int, [C.POINTER(Filter3dObserveArgs)]),
    "gsr_filter3d_finalize": (C.c_int, [C.POINTER(Filter3dFinalizeArgs)]),
    "gsr_filter3d_forward": (C.c_int, [C.POINTER(Filter3dArgs)]),
    "gsr_filter3d_backward": (C.c_int, [C.POINTER(Filter3dBackwardArgs)]),
}

# include/gsrast_amd_absgrad.h (AbsGS: the absolute screen-space gradient of a frame), in the same shape, with its own symbol test.
class AbsgradArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("backward", C.POINTER(BackwardArgs)),
                ("dL_dout_alpha", C.c_void_p), ("abs_dL_dmean2D", C.c_void_p), ("sums_f64", C.c_void_p), ("stage_ms", C.c_float)]


ABSGRAD_SIGNATURES = {
    "gsr_absgrad": (C.c_int, [C.POINTER(AbsgradArgs)]),
}

# include/gsrast_amd_features.h (N-channel feature maps of a drawn frame, forward and backward), in the same shape, with its own symbol test.
GSR_FEATURES_MAX_CHANNELS = 256
GSR_FEATURES_CHUNK = 16
GSR_FEATURES_CHUNK_NARROW = 8


class FeaturesArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("means2D", C.c_void_p), ("conic_opacity", C.c_void_p), ("ranges", C.c_void_p), ("n_contrib", C.c_void_p),
                ("final_t", C.c_void_p), ("point_list", C.c_void_p), ("receipt", ForwardReceipt),
                ("features", C.c_void_p), ("background", C.c_void_p), ("out", C.c_void_p),
                ("dL_dout", C.c_void_p), ("dL_dfeatures", C.c_void_p), ("feature_sums_f64", C.c_void_p),
                ("geometry_sums_f64", C.c_void_p),
                ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32), ("stream", C.c_void_p), ("stage_ms", C.c_float)]


FEATURES_SIGNATURES = {
    "gsr_features_temp_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gsr_features_forward": (C.c_int, [C.POINTER(FeaturesArgs)]),
    "gsr_features_backward": (C.c_int, [C.POINTER(FeaturesArgs)]),
}

# include/gsrast_amd_distortion.h (the depth distortion map of a drawn frame, forward and backward), in the same shape, with its own symbol test.
class DistortionArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("power", C.c_int32),
                ("means2D", C.c_void_p), ("conic_opacity", C.c_void_p), ("ranges", C.c_void_p), ("n_contrib", C.c_void_p),
                ("final_t", C.c_void_p), ("point_list", C.c_void_p), ("receipt", ForwardReceipt),
                ("values", C.c_void_p), ("out", C.c_void_p), ("moments", C.c_void_p),
                ("dL_dout", C.c_void_p), ("dL_dvalues", C.c_void_p), ("value_sums_f64", C.c_void_p),
                ("geometry_sums_f64", C.c_void_p),
                ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32), ("stream", C.c_void_p), ("stage_ms", C.c_float)]


DISTORTION_SIGNATURES = {
    "gsr_distortion_temp_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_distortion_forward": (C.c_int, [C.POINTER(DistortionArgs)]),
    "gsr_distortion_backward": (C.c_int, [C.POINTER(DistortionArgs)]),
}

# include/gsrast_amd_normals.h (the per-Gaussian normal and the normal of a depth surface, forward and backward), in the same shape, with its own symbol test.
_GAUSSIAN_NORMALS_COMMON = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("num_gaussians", C.c_int32),
                            ("means3D", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p), ("view_matrix", C.c_void_p)]
_DEPTH_NORMALS_COMMON = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("width", C.c_int32), ("height", C.c_int32),
                         ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("depth", C.c_void_p)]


class GaussianNormalsArgs(C.Structure):
    _fields_ = _GAUSSIAN_NORMALS_COMMON + [("normals", C.c_void_p), ("stream", C.c_void_p)]


class GaussianNormalsBackwardArgs(C.Structure):
    _fields_ = _GAUSSIAN_NORMALS_COMMON + [("dL_dnormals", C.c_void_p), ("radii", C.c_void_p), ("dL_drotations", C.c_void_p),
                                           ("stream", C.c_void_p)]


class DepthNormalsArgs(C.Structure):
    _fields_ = _DEPTH_NORMALS_COMMON + [("normals", C.c_void_p), ("stream", C.c_void_p)]


class DepthNormalsBackwardArgs(C.Structure):
    _fields_ = _DEPTH_NORMALS_COMMON + [("dL_dnormals", C.c_void_p), ("dL_ddepth", C.c_void_p), ("stream", C.c_void_p)]


NORMALS_SIGNATURES = {
    "gsr_gaussian_normals_forward": (C.c_int, [C.POINTER(GaussianNormalsArgs)]),
    "gsr_gaussian_normals_backward": (C.c_int, [C.POINTER(GaussianNormalsBackwardArgs)]),
    "gsr_depth_normals_forward": (C.c_int, [C.POINTER(DepthNormalsArgs)]),
    "gsr_depth_normals_backward": (C.c_int, [C.POINTER(DepthNormalsBackwardArgs)]),
}

# include/gsrast_amd_median.h (the median depth map and the per-pixel Gaussian ids of a drawn frame, forward and backward), in the same shape, with its own symbol test.
GSR_MEDIAN_NONE = 0xFFFFFFFF


class MedianArgs(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32),
                ("num_gaussians", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("threshold", C.c_float),
                ("means2D", C.c_void_p), ("conic_opacity", C.c_void_p), ("ranges", C.c_void_p), ("n_contrib", C.c_void_p),
                ("final_t", C.c_void_p), ("point_list", C.c_void_p), ("receipt", ForwardReceipt),
                ("values", C.c_void_p), ("out", C.c_void_p), ("ids", C.c_void_p), ("dominant_ids", C.c_void_p),
                ("dL_dout", C.c_void_p), ("dL_dvalues", C.c_void_p), ("value_sums_f64", C.c_void_p),
                ("tile_row_begin", C.c_int32), ("tile_row_end", C.c_int32), ("stream", C.c_void_p), ("stage_ms", C.c_float)]


MEDIAN_SIGNATURES = {
    "gsr_median_temp_bytes": (C.c_size_t, [C.c_int32]),
    "gsr_median_forward": (C.c_int, [C.POINTER(MedianArgs)]),
    "gsr_median_backward": (C.c_int, [C.POINTER(MedianArgs)]),
}

_lib = None


class GsrError(RuntimeError):
    def __init__(self, code: int, where: str):
        L = lib()
        msg = L.gsr_error_string(code).decode()
        hip = L.gsr_last_hip_error().decode()
        super().__init__(f"{where}: {msg} (code {code})" + (f" [{hip}]" if hip else ""))
        self.code = code


def lib() -> C.CDLL:
    """Loads libgsrast_amd.so. Raises if it has not been built: there is no CPU path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP library first (python -m gsrast_amd.build). "
                "gsrast_amd has no CPU or PyTorch fallback.")
        # PyTorch bundles its own libamdhip64.so.7; it must be the one already mapped when our
        # library resolves that soname, otherwise two HIP runtimes end up in the process and
        # torch's device pointers mean nothing to ours ("no HIP device"): this module imports torch first.
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in (list(SIGNATURES.items()) + list(INIT_SIGNATURES.items()) + list(OPACITY_SIGNATURES.items())
                                  + list(MCMC_SIGNATURES.items()) + list(CONTRIB_SIGNATURES.items()) + list(ANTIALIAS_SIGNATURES.items())
                                  + list(FILTER3D_SIGNATURES.items()) + list(ABSGRAD_SIGNATURES.items())
                                  + list(FEATURES_SIGNATURES.items()) + list(DISTORTION_SIGNATURES.items())
                                  + list(NORMALS_SIGNATURES.items()) + list(MEDIAN_SIGNATURES.items())):
            fn = getattr(L, name, None)
            if fn is None and _TAG:
                continue                       # (a tagged A/B build of an older tree may lack the newest entry points)
            if fn is None:
                raise RuntimeError(f"{LIB_PATH} does not export {name}: rebuild it (python -m gsrast_amd.build)")
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(code: int, where: str) -> None:
    if code != GSR_OK:
        raise GsrError(code, where)


def call(name: str, *args, device=None, where: "str | None" = None) -> None:
    """The entry point `name` (one that returns a GSR_* code), called with `device` current if one is given: GsrError unless GSR_OK."""
    fn = getattr(lib(), name)
    if device is None:
        code = fn(*args)
    else:
        with torch.cuda.device(device):
            code = fn(*args)
    check(code, where or name)


def stream(device) -> int:
    """torch's current stream on `device`, as the `stream` arguments of the C ABI take it."""
    return torch.cuda.current_stream(device).cuda_stream


def aligned16(t: torch.Tensor) -> torch.Tensor:
    """(the kernels move rows in 16-byte vectors: a strided view, or one that starts in the middle of a vector, is copied)"""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()
