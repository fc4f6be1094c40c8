"""CPU: the camera gradients' ABI (gsr_camera_backward, gsr_camera_backward_scratch_bytes) and the float64 reference the GPU
tests use (tests/camera_grad_ref.py), pinned by central differences of the float64 per-Gaussian forward functions of
oracle/backward_np.py w.r.t. each of the 35 camera floats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from camera_grad_ref import ZERO_ENTRIES, camera_terms, focal_lengths
from gsrast_amd import _capi
from test_depth_cpu import depth_values_f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in _capi.CameraBackwardArgs._fields_]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_camera_struct_matches_the_header(tmp_path):
    body = 'printf("size %zu\\n", sizeof(gsr_camera_backward_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_camera_backward_args, {f}));' for f in FIELDS)
    src, exe = tmp_path / "camera_abi.c", tmp_path / "camera_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.CameraBackwardArgs)
    for f in FIELDS:
        assert int(got[f]) == getattr(_capi.CameraBackwardArgs, f).offset, f


def test_camera_entry_points_are_exported():
    L = _capi.lib()
    for name in ("gsr_camera_backward", "gsr_camera_backward_scratch_bytes"):
        assert hasattr(L, name) and name in _capi.SIGNATURES, name


def _args():
    """A call that would be complete: every pointer it needs set (to an address no test dereferences — each case below is
    refused before the library touches memory or a device)."""
    a = _capi.CameraBackwardArgs()
    a.struct_size = C.sizeof(_capi.CameraBackwardArgs)
    a.num_gaussians, a.width, a.height = 100, 64, 48
    a.tan_fovx = a.tan_fovy = 0.4
    for f in ("means3D", "view_matrix", "proj_matrix", "cov3D", "radii", "dL_dmean2D", "dL_dcov2D", "dL_dview_matrix",
              "dL_dproj_matrix", "dL_dcam_pos", "scratch"):
        setattr(a, f, 0x10000)
    return a


def _unset(*names):
    return lambda a: [setattr(a, f, None) for f in names]


def _shs_without(missing):
    def edit(a):
        a.flags = _capi.GSR_FLAG_SEMANTICS_INRIA
        a.sh_dims = 3
        for f in ("shs", "clamped", "cam_pos", "dL_dcolors"):
            setattr(a, f, None if f == missing else 0x10000)
    return edit


REFUSALS = {
    "struct_size short": lambda a: setattr(a, "struct_size", C.sizeof(_capi.CameraBackwardArgs) - 8),
    "struct_size long": lambda a: setattr(a, "struct_size", C.sizeof(_capi.CameraBackwardArgs) + 8),
    "no gaussians": lambda a: setattr(a, "num_gaussians", 0),
    "no width": lambda a: setattr(a, "width", 0),
    "no height": lambda a: setattr(a, "height", -1),
    "no output": _unset("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos"),
    "shs without dL_dcolors": _shs_without("dL_dcolors"),
    "shs without clamped": _shs_without("clamped"),
    "shs without cam_pos": _shs_without("cam_pos"),
}
for _f in ("means3D", "view_matrix", "proj_matrix", "cov3D", "radii", "dL_dmean2D", "dL_dcov2D", "scratch"):
    REFUSALS[f"no {_f}"] = _unset(_f)


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_camera_backward_refuses_before_any_device_call(case):
    L = _capi.lib()
    a = _args()
    REFUSALS[case](a)
    assert L.gsr_camera_backward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG, case
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_camera_backward(None) == _capi.GSR_ERR_INVALID_ARG


def test_camera_scratch_depends_on_n_only():
    """One 256-byte row of double partials per block of the pass: ceil(N / 256) blocks, at most 768."""
    L = _capi.lib()
    assert L.gsr_camera_backward_scratch_bytes(0) == 0 and L.gsr_camera_backward_scratch_bytes(-5) == 0
    for n in (1, 255, 256, 257, 1200, 196_608, 196_609, 5_834_784, 50_000_000, 2**31 - 1):
        got = L.gsr_camera_backward_scratch_bytes(n)
        assert got == L.gsr_camera_backward_scratch_bytes(n) == 256 * min(768, -(-n // 256)), n


# ---- the reference against finite differences ---------------------------------------------------------------------------
def _scenario(sh_degree, seed, pose="default"):
    """Ten Gaussians in front of a 64 x 48 camera — two of them with t.x / t.z, t.y / t.z beyond 1.3 tan_fov, one with a
    colour channel clamped at zero — and one behind it (radius 0), with random per-Gaussian gradients. Everything the
    library reads as float32 is float32-representable. pose: "default" (no rotation: the view matrix's rotation block is
    diag(1, -1, 1)) or "posed" (rotated and rolled: the block is not symmetric); the three placed Gaussians sit at the same
    view-space positions under either."""
    from gsrast_amd import camera
    from helpers import posed_camera, world_from_view
    from oracle import backward_np as B
    rng = np.random.default_rng(seed)
    W, H = 64, 48
    if pose == "default":
        cam = camera.default_camera(W, H, near=0.05, far=50.0, position=(0.3, -0.2, -4.0))
    else:
        cam = posed_camera(W, H, eye=(2.0, -1.2, -4.2), target=0.0, roll=0.4)
    n = 11
    means = np.ones((n, 4))
    means[:, :3] = rng.uniform(-1.0, 1.0, size=(n, 3))
    # in view space (under the default pose: the world positions (6, 0.2, 0.3), (0.1, 4.5, -0.2) and (0, 0, -7))
    means[0, :3] = world_from_view(cam, [[5.7, -0.4, 4.3]])[0]     # far to the side: t.x / t.z clamped
    means[1, :3] = world_from_view(cam, [[-0.2, -4.7, 3.8]])[0]    # far up: t.y / t.z clamped
    means[10, :3] = world_from_view(cam, [[-0.3, -0.2, -3.0]])[0]  # behind the camera
    means = means.astype(np.float32).astype(np.float64)
    radii = np.ones(n, np.int32)
    radii[10] = 0
    M = rng.normal(size=(n, 3, 3)) * 0.15
    S = M @ M.transpose(0, 2, 1) + 0.01 * np.eye(3)
    cov3D = np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)
    shs = (0.4 * rng.normal(size=(n, 48))).astype(np.float32).astype(np.float64)
    shs[2, 0] = -4.0                        # Gaussian 2: channel 0 clamped at zero (its other coefficients made small)
    shs[2, 3::3] = (0.1 * shs[2, 3::3]).astype(np.float32)
    grads = dict(dL_dmean2D=rng.normal(size=(n, 2)), dL_dcov2D=np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1),
                 dL_ddepths=rng.normal(size=n) * 3.0, dL_dcolors=rng.normal(size=(n, 3)))
    clamped = np.zeros((n, 3), bool)
    for i in range(n):
        v = means[i, :3] - np.asarray(cam.cam_pos, np.float64)
        Bk, _ = B.sh_basis(v / np.linalg.norm(v), sh_degree)
        clamped[i] = Bk @ shs[i].reshape(16, 3) + 0.5 < 0.0
    assert clamped[2, 0]
    return cam, means, radii, cov3D, shs, grads, clamped


def _per_gaussian_loss(inria, sh_degree, depth, cam, mean3, c3, sh, g):
    """F(camera floats) of one Gaussian: its share of L through the pixel centre, cov2D, depth and (upstream) colour."""
    from oracle import backward_np as B
    W, H = cam.width, cam.height
    fx, fy = focal_lengths(W, H, cam.tan_fovx, cam.tan_fovy, inria, f32=False)
    gM = np.array([[g["dL_dcov2D"][0], g["dL_dcov2D"][1]], [g["dL_dcov2D"][1], g["dL_dcov2D"][2]]])

    def F(x):
        view, proj, cam_pos = x[:16], x[16:32], x[32:35]
        if inria:
            mean2D = B.inria_project_mean2d(mean3, proj, W, H)
            J, Wm, _, _ = B._inria_jw(mean3, view, fx, fy, cam.tan_fovx, cam.tan_fovy)
            P = J @ Wm
        else:
            mean2D = B.project_mean2d(mean3, proj, W, H)
            P = B._jw(mean3, view, fx, cam.tan_fovx, cam.tan_fovy)
        f = float(g["dL_dmean2D"] @ mean2D) + float((gM * (P @ B._sigma(c3) @ P.T)).sum())
        if depth:
            f += float(g["dL_ddepths"] * depth_values_f64(mean3, view, depth == "inverse"))
        if inria:
            f += float(g["dL_dcolors"] @ B.inria_color(mean3, cam_pos, sh, sh_degree))
        return f
    return F


CASES = [("gscuda", None, 0), ("gscuda", True, 0), ("gscuda", "inverse", 0), ("gscuda", True, 3),
         ("inria", None, 0), ("inria", True, 3), ("inria", "inverse", 3), ("inria", None, 1), ("inria", True, 2)]


@pytest.mark.parametrize("semantics,depth,sh_degree", CASES)
def test_camera_reference_against_central_differences(semantics, depth, sh_degree):
    """Every visible Gaussian's 35 terms against central differences of its share of L, taken w.r.t. each camera float;
    exact zeros where nothing depends on the entry; the float32-decision variant (what the kernel does) within 1e-5."""
    _reference_against_central_differences(semantics, depth, sh_degree, "default")


@pytest.mark.parametrize("semantics,depth,sh_degree", CASES)
def test_camera_reference_against_central_differences_under_a_rotated_pose(semantics, depth, sh_degree):
    """The same under a rotated and rolled camera (the test above keeps its ids): there the view matrix's rotation block is
    not symmetric, so that the reference's own indexing of it is pinned too."""
    _reference_against_central_differences(semantics, depth, sh_degree, "posed")


def _reference_against_central_differences(semantics, depth, sh_degree, pose):
    from oracle import backward_np as B
    inria = semantics == "inria"
    cam, means, radii, cov3D, shs, grads, clamped = _scenario(sh_degree, seed=len(semantics) + sh_degree + 7, pose=pose)
    kw = dict(dL_ddepths=grads["dL_ddepths"] if depth else None, inverse=depth == "inverse", inria=inria,
              shs=shs, sh_degree=sh_degree, dL_dcolors=grads["dL_dcolors"], clamped=clamped)
    args = (means, cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, radii, cov3D,
            grads["dL_dmean2D"], grads["dL_dcov2D"])
    vis, T = camera_terms(*args, f32_decisions=False, **kw)
    vis, T = vis.numpy(), T.numpy()
    assert list(vis) == list(range(10))                    # the Gaussian behind the camera contributes nothing
    x0 = np.concatenate([np.asarray(cam.view, np.float64), np.asarray(cam.proj, np.float64),
                         np.asarray(cam.cam_pos, np.float64)])
    # the clamped cases are there (float64 decisions, as the finite differences see them)
    v = x0[:16]
    t = np.array([[v[r] * m[0] + v[4 + r] * m[1] + v[8 + r] * m[2] + v[12 + r] for r in range(3)] for m in means[:10, :3]])
    assert abs(t[0, 0] / t[0, 2]) > 1.3 * cam.tan_fovx and abs(t[1, 1] / t[1, 2]) > 1.3 * cam.tan_fovy
    assert (t[:, 2] > 0.2).all()
    tb = [v[r] * means[10, 0] + v[4 + r] * means[10, 1] + v[8 + r] * means[10, 2] + v[12 + r] for r in range(3)]
    assert tb[2] < -1.0                                    # Gaussian 10 is behind the camera under either pose
    for j, i in enumerate(vis):
        g = {k: grads[k][i] for k in grads}
        F = _per_gaussian_loss(inria, sh_degree, depth, cam, means[i, :3], cov3D[i], shs[i].reshape(16, 3), g)
        fd = B.finite_difference(F, x0, 1e-6)
        scale = float(np.abs(fd).max())
        err = np.abs(T[j] - fd)
        assert (err <= 1e-6 * scale).all(), (i, np.nonzero(err > 1e-6 * scale)[0], err.max(), scale)
    assert (T[:, ZERO_ENTRIES] == 0).all()
    if not inria or sh_degree == 0:
        assert (T[:, 32:35] == 0).all()
    else:
        assert np.abs(T[:, 32:35]).max() > 0
        # the clamped channel passes nothing: a colour gradient in that channel alone gives Gaussian 2 no cam_pos term
        g0 = dict(kw, dL_dcolors=np.where(np.arange(3) == 0, grads["dL_dcolors"], 0.0))
        T0 = camera_terms(*args, f32_decisions=False, **g0)[1].numpy()
        assert (T0[2, 32:35] == 0).all() and np.abs(T0[3:, 32:35]).max() > 0
    if depth is None:
        Td = camera_terms(*args, f32_decisions=False, **dict(kw, dL_ddepths=grads["dL_ddepths"]))[1].numpy()
        row2 = [2, 6, 10, 14]
        assert np.abs(Td[:, row2] - T[:, row2]).max() > 0            # the depth term moves view row 2 only
        assert np.array_equal(np.delete(Td, row2, 1), np.delete(T, row2, 1))
    T32 = camera_terms(*args, f32_decisions=True, **kw)[1].numpy()
    M = np.abs(T).sum(0)
    assert (np.abs(T32.sum(0) - T.sum(0)) <= 1e-5 * M).all()
