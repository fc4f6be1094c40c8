"""Initial Gaussians from a point cloud: the role of upstream's create_from_pcd, where a 3DGS training run begins.

    params = GaussianParams.from_points_ply("sparse/0/points3D.ply")       # or from_points(xyz, rgb)

  knn_mean_dist2   per point, the mean squared distance to its three nearest neighbours: simple_knn's distCUDA2, exact, in HIP
                   (gsr_knn_mean_dist2, csrc/knn.hip; include/gsrast_amd_init.h states the result operation by operation)
  initial_values   upstream's initial raw values from positions and colours
"""
from __future__ import annotations

import math

import torch

from . import _capi

SH_C0 = 0.28209479177387814
INITIAL_OPACITY = 0.1
MIN_DIST2 = 1e-7


def _refuse_xyz(xyz, where: str) -> None:
    if not isinstance(xyz, torch.Tensor):
        raise ValueError(f"{where}: xyz is a {type(xyz).__name__}, not a tensor")
    if xyz.dtype != torch.float32:
        raise ValueError(f"{where}: xyz is {xyz.dtype}, not float32")
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"{where}: xyz is {tuple(xyz.shape)}, not [N, 3]")
    if not xyz.is_cuda:
        raise ValueError(f"{where}: xyz is on {xyz.device}, not on a GPU")
    if xyz.shape[0] > _capi.GSR_KNN_MAX_POINTS:
        raise ValueError(f"{where}: {xyz.shape[0]} points, more than {_capi.GSR_KNN_MAX_POINTS}")


def knn_mean_dist2(xyz: torch.Tensor) -> torch.Tensor:
    """f32[N]: for every row of xyz (float32 [N,3] on a GPU; a non-contiguous one is copied) the mean of the squared
    distances to its three nearest other rows, a duplicate row being a neighbour at distance 0; with fewer than four rows
    the mean over the rows there are, and +0 for a single one (upstream sums FLT_MAX placeholders there). Exact, and a
    pure function of xyz: bit for bit the brute force of include/gsrast_amd_init.h. Coordinates must be finite.

    The result and the call's scratch are new tensors; everything is enqueued on the current stream of xyz's device and
    nothing synchronises. ValueError before anything is launched: xyz not a float32 [N,3] tensor on a GPU."""
    _refuse_xyz(xyz, "knn_mean_dist2")
    n, dev = int(xyz.shape[0]), xyz.device
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    xyz = xyz.detach().contiguous()
    temp = torch.empty(int(_capi.lib().gsr_knn_temp_bytes(n)), dtype=torch.uint8, device=dev)
    _capi.call("gsr_knn_mean_dist2", n, xyz.data_ptr(), out.data_ptr(), temp.data_ptr(), _capi.stream(dev), device=dev)
    # (temp goes back to torch's caching allocator here, which hands it out again on this stream only: behind the call)
    return out


def initial_values(xyz: torch.Tensor, rgb: torch.Tensor):
    """Upstream's create_from_pcd values for points xyz (float32 [N,3] on a GPU) with colours rgb (float32 [N,3] in [0, 1],
    same device): (xyz, opacity_logit [N], log_scale [N,3], rotation [N,4], shs [N,48]) — the order GaussianParams takes.

      xyz            unchanged (the same tensor)
      opacity_logit  log(0.1 / 0.9) everywhere
      log_scale      log(sqrt(clamp_min(knn_mean_dist2(xyz), 1e-7))), the same on the three axes
      rotation       (1, 0, 0, 0)
      shs            the DC triple (rgb - 0.5) / 0.28209479177387814, zeros elsewhere (the DC triple comes first in both
                     SH layouts, so the result is valid for either)

    Apart from knn_mean_dist2 these are plain torch operations, deliberately: they run once per training run and move 59
    floats per point, and the device has no pinned logf a fused kernel could be held to bit for bit. No kernel of the
    library's own stands behind them."""
    _refuse_xyz(xyz, "initial_values")
    n, dev = int(xyz.shape[0]), xyz.device
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.float32 or tuple(rgb.shape) != (n, 3) or rgb.device != dev:
        what = f"{rgb.dtype} {tuple(rgb.shape)} on {rgb.device}" if isinstance(rgb, torch.Tensor) else type(rgb).__name__
        raise ValueError(f"initial_values: rgb is {what}, not float32 {(n, 3)} on {dev}")
    dist2 = knn_mean_dist2(xyz)
    log_scale = torch.log(torch.sqrt(torch.clamp_min(dist2, MIN_DIST2)))[:, None].repeat(1, 3)
    rotation = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rotation[:, 0] = 1.0
    opacity_logit = torch.full((n,), math.log(INITIAL_OPACITY / (1.0 - INITIAL_OPACITY)), dtype=torch.float32, device=dev)
    shs = torch.zeros((n, 48), dtype=torch.float32, device=dev)
    shs[:, 0:3] = (rgb - 0.5) / SH_C0
    return xyz, opacity_logit, log_scale, rotation, shs
