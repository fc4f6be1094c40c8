"""GPU: the backward passes under rotated cameras and at the chain's edges. Every other backward test renders through
camera.default_camera, whose view matrix has the rotation block diag(1, -1, 1) and focal_x == focal_y: there a transposed
rotation index, a dropped off-diagonal term of W Sigma W^T, a depth term read from a column instead of a row, and
focal_x / focal_y exchanged all give the same numbers. Here the per-Gaussian chain (preprocess_backward_kernel, both
profiles) and the camera pass (camera_pass_kernel) are checked against the float64 oracle (oracle/backward_np.py,
tests/camera_grad_ref.py; both pinned under a rotated pose by finite differences on the CPU) under two rotated and rolled
poses, with non-square pixels, with Gaussians beyond the +-1.3 tan(fov) clamp, with scale_modifier != 1, and at the tails
of the SH gradient's LDS staging.

Each case carries a blindness guard: the reference is computed a second time from inputs with the fault built in that the
case exists for, and must then differ from the true reference by more than ten times the case's tolerance — per Gaussian,
on its own largest component, on at least a quarter of the Gaussians checked (on every one for the clamp). No tolerance
here is new: each is the one the corresponding default-pose test or helper uses."""
import functools

import numpy as np
import pytest

from camera_grad_ref import ZERO_ENTRIES, camera_grad, camera_terms
from test_depth_cpu import depth_mean_term, depth_values_f32

pytestmark = pytest.mark.gpu

RTOL = 2e-4       # as tests/test_gpu_backward.py: float32 sums in some order against float64
W, H, N = 96, 64, 800
BG = (0.2, 0.5, 0.9)
POSES = {"P1": dict(eye=(2.0, -1.2, -4.2), target=(0.0, 0.0, 0.0), roll=0.4),
         "P2": dict(eye=(-1.5, 2.0, 3.5), target=(0.2, 0.0, 0.0), roll=-0.7)}       # P2 looks from behind the scene
CAM_KEYS = ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")
CHAIN_KEYS = ("dL_dcov3D", "dL_dmeans3D", "dL_dscales", "dL_drotations")


def _camera(pose, w=W, h=H, kx=1.0):
    from helpers import posed_camera, view_rotation
    cam = posed_camera(w, h, kx=kx, **POSES[pose])
    R = view_rotation(cam)
    assert np.abs(R - R.T).max() > 0.1                      # the branch these tests exist for: no symmetric rotation block
    return cam


def _scene(profile, n, seed):
    """scenes.garden_like_scene shrunk by 0.25; the upstream profile with all sixteen SH triples and quaternions that are
    not unit (the profile does not normalise), as test_backward_of_the_upstream_profile_matches_float64_oracle."""
    from gsrast_amd import scenes
    scene = scenes.garden_like_scene(n, seed=seed)
    scene["means3D"][:, :3] *= 0.25
    if profile == "inria":
        rng = np.random.default_rng(seed)
        scene["shs"] = rng.normal(0, 0.35, (n, 48)).astype(np.float32)
        scene["rotations"] *= rng.uniform(0.7, 1.4, (n, 1)).astype(np.float32)
    return scene


def _close(got, exp, what, rtol=RTOL):
    scale = max(1e-6, float(np.abs(exp).max()))
    err = float(np.abs(np.asarray(got, np.float64) - exp).max())
    assert err <= rtol * scale, f"{what}: max abs err {err} at scale {scale}"


def _state(r):
    import ctypes as C
    import torch
    from gsrast_amd import _capi
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    plist = r.map_binning_state()["values"].cpu().numpy().view(np.uint32).astype(np.int64)
    st = _capi.GeometryState()
    r.lib.gsr_geometry_from_chunk(r.geom.base(), r.num_gaussians, C.byref(st))
    clamped = r.geom.view(st.clamped, 3 * r.num_gaussians, torch.uint8).cpu().numpy().reshape(-1, 3).astype(bool)
    clamped[g["radii"] <= 0] = False
    return g, im, plist, clamped


def _numpy(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _assert_seen_enough(vis, scene_n, r):
    assert r.last_num_rendered > 0
    assert vis.size >= scene_n / 2, (vis.size, scene_n)     # the pose looks at the scene: at least half of it has a tile


def _rasterizer(scene, cam, bg=BG):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, background=bg)
    r.configure_from_scene(scene)
    return r


def _kw(profile, deg=None):
    return dict(semantics=profile, sh_degree=(3 if deg is None else deg) if profile == "inria" else 0)


def _expected_chain(profile, got, g, scene, cam, ids, clamped, deg=3, **kw):
    from helpers import backward_chain_expected, backward_chain_expected_inria
    if profile == "inria":
        return backward_chain_expected_inria(got, g, scene, cam, cam.width, cam.height, ids, deg, clamped, **kw)
    return backward_chain_expected(got, g, scene, cam, cam.width, cam.height, ids, **kw)


def _check_chain(profile, got, g, scene, cam, ids, clamped, deg=3, **kw):
    from helpers import check_backward_chain, check_backward_chain_inria
    if profile == "inria":
        return check_backward_chain_inria(got, g, scene, cam, cam.width, cam.height, ids, deg, clamped, **kw)
    return check_backward_chain(got, g, scene, cam, cam.width, cam.height, ids, **kw)


def _assert_culled_zero(profile, got, g):
    culled = g["radii"] <= 0
    for k in CHAIN_KEYS + (("dL_dshs",) if profile == "inria" else ()):
        assert (got[k][culled] == 0).all(), k


def _guard_share(seen, what, share=0.25):
    """A fault's reference differs from the true one where `seen`: that must be at least `share` of the Gaussians checked —
    a condition on the case (pose, scene), not a measurement of the code under test."""
    assert seen.size > 0 and seen.mean() >= share, f"{what}: the fault would be seen on {int(seen.sum())} of {seen.size} Gaussians only"


# ---- one frame per (profile, pose, kx): forward state, gradients, and the float64 blend reference, shared by the cases ----
@functools.lru_cache(maxsize=None)
def _frame(profile, pose, kx=1.0):
    import torch
    from oracle import backward_np as B
    scene = _scene(profile, N, seed=4)
    cam = _camera(pose, kx=kx)
    r = _rasterizer(scene, cam)
    kw = _kw(profile)
    img = r.draw(cam, plan="sort", tile_history=False, **kw).cpu().numpy().copy()
    g, im, plist, clamped = _state(r)
    rng = np.random.default_rng(17)
    dL = rng.normal(size=(3, H, W)).astype(np.float32)
    got = _numpy(r.backward(torch.from_numpy(dL), wide_sums=True, **kw))
    ranges = im["ranges"].view(np.uint32).astype(np.int64)
    cut = 1e-4 if profile == "inria" else 0.001
    out64, ft64, nc64 = B.blend_forward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, W, H, BG, t_cutoff=cut)
    assert np.abs(out64 - img).max() <= 1e-4
    assert (nc64 != im["nContrib"].view(np.uint32)).sum() <= 2
    exp = B.blend_backward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, nc64, ft64, W, H, BG, dL)
    vis = np.nonzero(g["radii"] > 0)[0]
    _assert_seen_enough(vis, N, r)
    return dict(scene=scene, cam=cam, r=r, g=g, im=im, plist=plist, clamped=clamped, dL=dL, got=got, ranges=ranges,
                nc64=nc64, ft64=ft64, exp=exp, vis=vis, kw=kw)


def _check_frame(f, profile, what, guard):
    """The render backward against the float64 blend backward, then the chain for every visible Gaussian, exact zeros for
    the others, and the case's blindness guard: guard(cam) -> kwargs / camera of the faulted reference."""
    from helpers import chain_seen
    got, exp, g, cam, scene, vis = f["got"], f["exp"], f["g"], f["cam"], f["scene"], f["vis"]
    _close(got["dL_dmean2D"], exp["dL_dmean2D"], what + ": dL_dmean2D")
    _close(got["dL_dconic_opacity"][:, :3], exp["dL_dconic"], what + ": dL_dconic")
    _close(got["dL_dconic_opacity"][:, 3], exp["dL_dopacity"], what + ": dL_dopacity")
    _close(got["dL_dcolors"], exp["dL_dcolor"], what + ": dL_dcolors")
    assert np.abs(exp["dL_dmean2D"]).max() > 0 and np.abs(exp["dL_dconic"]).max() > 0
    e = _expected_chain(profile, got, g, scene, cam, vis, f["clamped"])
    mags = _check_chain(profile, got, g, scene, cam, vis, f["clamped"], expected=e)
    assert all(m > 0 for m in mags)
    _assert_culled_zero(profile, got, g)
    if profile == "inria":
        assert f["clamped"][vis].any()                      # the colour clamp is exercised
    fault_cam, fault_kw = guard(cam)
    faulted = _expected_chain(profile, got, g, scene, fault_cam, vis, f["clamped"], **fault_kw)
    _guard_share(chain_seen(e, faulted), what)


def _transposed(cam):
    from helpers import with_transposed_rotation
    return with_transposed_rotation(cam), {}


# ---- a. the chain under rotation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pose", ["P1", "P2"])
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_chain_under_a_rotated_pose(profile, pose):
    """Both profiles under P1 and P2 (wide_sums=True): the sums against B.blend_backward, the chain of every visible
    Gaussian against the oracle at the helpers' per-Gaussian tolerances. Guard: the oracle fed a view matrix whose rotation
    block is transposed."""
    _check_frame(_frame(profile, pose), profile, f"{profile}/{pose}", _transposed)


def _well_conditioned(ref, min_share=0.05):
    """The Gaussians of oracle_gradients' result whose mean and covariance sums are not cancellations: |sum| >= min_share M
    on the sum's largest component. The float32 terms of a sum err by ~1e-7 (k + 8) M (helpers.BW_TAU), i.e. by at most
    2e-6 (k + 8) of such a sum — far inside the chain's 3e-3 —, whereas a sum that cancels to 1e-4 of M has no digits left
    to compare end to end. The choice is made from the reference alone."""
    ok = ref["pixels"] > 0
    for k in ("dL_dmean2D", "dL_dcov2D"):
        s, m = np.abs(ref["exp"][k]).max(1), ref["M"][k].max(1)
        ok &= s >= min_share * m
    return ok


@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_chain_end_to_end_under_a_rotated_pose(profile):
    """P1, the chain fed with sums computed in float64 on the host (helpers.oracle_gradients over every tile: the float32
    forward's decisions, float64 sums) instead of the GPU's: what the GPU returns for means3D, scales and rotations against a
    reference that shares nothing with it but the forward state. Guard: the transposed rotation block."""
    import torch
    from helpers import chain_seen, oracle_gradients
    f = _frame(profile, "P1")
    r, vis, got = f["r"], f["vis"], f["got"]
    tiles = [(tx, ty) for ty in range((H + 15) // 16) for tx in range((W + 15) // 16)]
    bad = []
    ref = oracle_gradients(r, torch.from_numpy(f["dL"]), BG, tiles, vis, max_depth=N, bad_pixels=bad, f32_forward=True,
                           magnitudes=True, t_cutoff=1e-4 if profile == "inria" else 0.001, full_lists=True)
    # a pixel on which the two forwards disagree (a record at a hard threshold) spoils the sums of its tile's Gaussians
    spoiled = set()
    for y, x in bad:
        t = (y // 16) * ((W + 15) // 16) + x // 16
        spoiled.update(int(i) for i in f["plist"][f["ranges"][t, 0]:f["ranges"][t, 1]])
    assert len(bad) <= 2, bad
    keep = _well_conditioned(ref) & ~np.isin(vis, sorted(spoiled))
    ids = vis[keep]
    assert ids.size >= 100, ids.size
    e = ref["exp"]
    up = {k: np.zeros((N, d)) for k, d in (("dL_dmean2D", 2), ("dL_dconic_opacity", 4), ("dL_dcov2D", 3), ("dL_dcolors", 3))}
    up["dL_dmean2D"][vis] = e["dL_dmean2D"]
    up["dL_dconic_opacity"][vis] = np.concatenate([e["dL_dconic"], e["dL_dopacity"]], 1)
    up["dL_dcov2D"][vis] = e["dL_dcov2D"]
    up["dL_dcolors"][vis] = e["dL_dcolors"]
    exp = _expected_chain(profile, got, f["g"], f["scene"], f["cam"], ids, f["clamped"], upstream=up)
    mags = _check_chain(profile, got, f["g"], f["scene"], f["cam"], ids, f["clamped"], upstream=up, expected=exp)
    assert all(m > 0 for m in mags)
    faulted = _expected_chain(profile, got, f["g"], f["scene"], _transposed(f["cam"])[0], ids, f["clamped"], upstream=up)
    exp.pop("dL_dshs", None), faulted.pop("dL_dshs", None)
    # (the rotation gradient is checked at ten times the others' tolerance end to end: it is left out of the guard)
    exp.pop("dL_drotations"), faulted.pop("dL_drotations")
    _guard_share(chain_seen(exp, faulted), f"{profile}: end to end")


# ---- b. non-square pixels in the upstream profile's backward ------------------------------------------------------------
@pytest.mark.parametrize("kx", [1.7, 0.55])
def test_upstream_chain_with_non_square_pixels(kx):
    """inria at P1 with tan_fovx = kx tan_fovy W / H: focal_x != focal_y in the chain's Jacobian. Guard: the oracle with the
    two focal lengths exchanged."""
    f = _frame("inria", "P1", kx)
    cam = f["cam"]
    fx, fy = W / (2.0 * cam.tan_fovx), H / (2.0 * cam.tan_fovy)
    assert abs(fx / fy - 1.0 / kx) < 1e-3                   # the factor is there
    _check_frame(f, "inria", f"inria/P1/kx={kx}", lambda c: (c, dict(swap_focal=True)))


# ---- c. the depth term under rotation ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [True, "inverse"])
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_depth_term_under_a_rotated_pose(profile, mode):
    """As test_depth_backward_matches_the_float64_superposition, at P1: dL_ddepths is the colour gradient of a blend of
    colours (d_i, 0, 0); dL_dmeans3D is the chain of the summed 2-D gradients plus dL_ddepths times ROW 2 of the view
    matrix, (V[2], V[6], V[10]). Guard: the term taken from the column (V[8], V[9], V[10]) — equal under the default pose."""
    import torch
    from helpers import _rows_differ
    from oracle import backward_np as B
    f = _frame(profile, "P1")
    r, g, cam, scene, vis, exp_c = f["r"], f["g"], f["cam"], f["scene"], f["vis"], f["exp"]
    inverse = mode == "inverse"
    # dL_ddepth: smooth and of one sign, as a depth loss gives it, of the colour gradient's size in view-space units (an
    # inverse depth is ~1 / |eye|^2 of a length). Under the white noise the default-pose test uses the direct term is 1 % of
    # dL_dmeans3D, and the row-for-column fault below would be seen on 1 to 15 % of the Gaussians only (measured on the
    # float64 reference alone); under this one it is 10 to 30 %, and the fault is seen on 57 to 61 %.
    amp = float(np.linalg.norm(cam.cam_pos)) ** 2 if inverse else 1.0
    gd = (amp * (1.0 + 0.25 * np.random.default_rng(23).normal(size=(H, W)))).astype(np.float32)
    got = _numpy(r.backward(torch.from_numpy(f["dL"]), dL_ddepth=torch.from_numpy(gd), depth=mode, wide_sums=True, **f["kw"]))
    d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), inverse).astype(np.float64)
    g3 = np.zeros((3, H, W))
    g3[0] = gd
    exp_d = B.blend_backward(g["means2D"], g["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), f["ranges"], f["plist"],
                             f["nc64"], f["ft64"], W, H, (0.0, 0.0, 0.0), g3)
    what = f"{profile}/{mode}"
    _close(got["dL_ddepths"], exp_d["dL_dcolor"][:, 0], f"{what}: dL_ddepths")
    _close(got["dL_dcolors"], exp_c["dL_dcolor"], f"{what}: dL_dcolors")
    _close(got["dL_dmean2D"], exp_c["dL_dmean2D"] + exp_d["dL_dmean2D"], f"{what}: dL_dmean2D")
    _close(got["dL_dconic_opacity"][:, :3], exp_c["dL_dconic"] + exp_d["dL_dconic"], f"{what}: dL_dconic")
    _close(got["dL_dconic_opacity"][:, 3], exp_c["dL_dopacity"] + exp_d["dL_dopacity"], f"{what}: dL_dopacity")
    assert np.abs(exp_d["dL_dcolor"][:, 0]).max() > 0 and np.abs(exp_d["dL_dmean2D"]).max() > 0
    assert (got["dL_ddepths"][g["radii"] <= 0] == 0).all()
    view32 = np.asarray(cam.view, np.float32)
    term = depth_mean_term(scene["means3D"][:, :3], view32, got["dL_ddepths"], inverse)
    chain = dict(got)
    chain["dL_dmeans3D"] = got["dL_dmeans3D"].copy()
    chain["dL_dmeans3D"][:, :3] -= term
    e = _expected_chain(profile, chain, g, scene, cam, vis, f["clamped"])
    _check_chain(profile, chain, g, scene, cam, vis, f["clamped"], expected=e)
    assert float(np.abs(term[vis]).max()) > 1e-3 * float(np.abs(got["dL_dmeans3D"][vis, :3]).max())
    # the guard: row and column of the view matrix differ here, and the difference is one the means3D check would see
    V = np.asarray(cam.view, np.float64)
    row, col = np.array([V[2], V[6], V[10]]), np.array([V[8], V[9], V[10]])
    assert np.abs(row - col).max() > 0.1
    term_col = (term @ row / (row @ row))[:, None] * col[None, :]      # the same dL/dz along the column instead
    full = e["dL_dmeans3D"] + term[vis]
    _guard_share(_rows_differ(full, e["dL_dmeans3D"] + term_col[vis], 10 * 3e-3), what)


# ---- d. the camera gradients under rotation ------------------------------------------------------------------------------
def _cam_vector(out):
    return np.concatenate([np.asarray(out[k]) for k in CAM_KEYS])


def _camera_reference(f_or_r, cam, grads, clamped, profile, mode, sh_degree, view=None):
    r = f_or_r
    g = r.map_geometry_state()
    inria = profile == "inria"
    args = (r.means3D, cam.view if view is None else view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, cam.width,
            cam.height, g["radii"], g["cov3D"], grads["dL_dmean2D"], grads["dL_dcov2D"])
    kw = dict(dL_ddepths=grads["dL_ddepths"] if mode else None, inverse=mode == "inverse", inria=inria,
              shs=r.shs if inria else None, sh_degree=sh_degree, dL_dcolors=grads["dL_dcolors"] if inria else None,
              clamped=clamped if inria else None)
    return args, kw


def _assert_camera_close(got, exp, M, what, rtol=1e-6):
    """tests/test_gpu_camera_grad.py's _assert_close: |err_k| <= rtol M_k + 1e-12 max M, ZERO_ENTRIES exact zeros."""
    assert np.isfinite(got).all(), what
    assert (got[ZERO_ENTRIES] == 0).all() and (got[M == 0] == 0).all(), f"{what}: entries without support are not zeros"
    err = np.abs(got.astype(np.float64) - exp)
    bad = err > rtol * M + 1e-12 * M.max()
    assert not bad.any(), f"{what}: entries {np.nonzero(bad)[0]}: err {err[bad]} > {rtol} x M {M[bad]}"


def _check_camera(r, cam, out, clamped, profile, mode, what, rtol=1e-6):
    """backward(camera=True)'s 35 floats against the float64 reference on the arrays the same call returned. Guard: the
    reference with the view's rotation block transposed differs — per Gaussian in its 35 terms by more than 10 rtol of the
    Gaussian's largest term on a quarter of the visible ones, and in the sums by more than 10 rtol M_k on some entry."""
    from helpers import _rows_differ, with_transposed_rotation
    sh_degree = 3 if profile == "inria" else 0
    got = _cam_vector(out)
    args, kw = _camera_reference(r, cam, out, clamped, profile, mode, sh_degree)
    T = camera_terms(*args, **kw)[1].numpy()
    exp, M = T.sum(0), np.abs(T).sum(0)
    _assert_camera_close(got, exp, M, what, rtol)
    assert M[:16].max() > 0 and M[16:32].max() > 0
    assert (M[32:] > 0).all() if profile == "inria" else (got[32:] == 0).all(), what
    args_t, _ = _camera_reference(r, cam, out, clamped, profile, mode, sh_degree, view=with_transposed_rotation(cam).view)
    Tt = camera_terms(*args_t, **kw)[1].numpy()
    assert Tt.shape == T.shape                               # (the visible set comes from radii, not from the view)
    _guard_share(_rows_differ(T, Tt, 10 * rtol), what)
    assert (np.abs(Tt.sum(0) - exp) > 10 * rtol * M + 1e-12 * M.max()).any(), what
    return exp, M


@functools.lru_cache(maxsize=None)
def _camera_setup(profile, pose):
    """As tests/test_gpu_camera_grad.py's _setup (SH coefficients beyond the DC term under either profile), at `pose`."""
    scene = _scene(profile, N, seed=2)
    if profile != "inria":
        scene["shs"][:, 3:] = 0.3 * np.random.default_rng(102).normal(size=(N, 45)).astype(np.float32)
    cam = _camera(pose)
    rng = np.random.default_rng(11)
    dL = rng.normal(size=(3, H, W)).astype(np.float32)
    gd = rng.normal(size=(H, W)).astype(np.float32)
    return scene, cam, _rasterizer(scene, cam), dL, gd


CAMERA_CASES = [(p, s, m, f, w) for p in ("P1", "P2") for s in ("gscuda", "inria") for m in (False, "inverse")
                for f in ("sorted", "block_lists") for w in (True, False)]


@pytest.mark.parametrize("pose,profile,mode,feed,wide", CAMERA_CASES)
def test_camera_grad_under_a_rotated_pose(pose, profile, mode, feed, wide):
    """|err_k| <= 1e-6 M_k against camera_grad_ref on the library's own per-Gaussian gradients, ZERO_ENTRIES exact, as
    test_camera_grad_matches_the_reference_on_the_librarys_own_gradients — under P1 and P2."""
    import torch
    scene, cam, r, dL, gd = _camera_setup(profile, pose)
    kw = _kw(profile)
    if feed == "sorted":
        r.draw(cam, plan="sort", tile_history=False, **kw)
    else:
        r.draw(cam, plan="blocks", sorted_lists=False, tile_history=False, **kw)
        assert not r.last_lists_written
    g, _, _, clamped = _state(r)
    _assert_seen_enough(np.nonzero(g["radii"] > 0)[0], N, r)
    out = _numpy(r.backward(torch.from_numpy(dL), dL_ddepth=torch.from_numpy(gd) if mode else None, depth=mode or None,
                            wide_sums=wide, camera=True, **kw))
    assert set(CAM_KEYS) <= set(out) and out["dL_dview_matrix"].shape == (16,) and out["dL_dcam_pos"].shape == (3,)
    _check_camera(r, cam, out, clamped, profile, mode, f"{pose}/{profile}/{mode}/{feed}/wide={wide}")


@pytest.mark.parametrize("profile,mode", [("gscuda", False), ("inria", "inverse")])
def test_camera_grad_end_to_end_under_a_rotated_pose(profile, mode):
    """As test_camera_grad_end_to_end_against_the_float64_blend_backward, at P1: the camera gradient against the float64
    reference applied to per-Gaussian gradients summed in float64 over the pixels, within 2e-4 of the largest entry."""
    import torch
    from helpers import with_transposed_rotation
    from oracle import backward_np as B
    f = _frame(profile, "P1")
    r, g, cam, scene = f["r"], f["g"], f["cam"], f["scene"]
    gd = np.random.default_rng(23).normal(size=(H, W)).astype(np.float32)
    out = _numpy(r.backward(torch.from_numpy(f["dL"]), dL_ddepth=torch.from_numpy(gd) if mode else None, depth=mode or None,
                            camera=True, **f["kw"]))
    got = _cam_vector(out)
    e = f["exp"]
    d_mean, d_conic, dd = e["dL_dmean2D"], e["dL_dconic"], None
    if mode:
        d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), mode == "inverse").astype(np.float64)
        g3 = np.zeros((3, H, W))
        g3[0] = gd
        ed = B.blend_backward(g["means2D"], g["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), f["ranges"], f["plist"],
                              f["nc64"], f["ft64"], W, H, (0.0, 0.0, 0.0), g3)
        d_mean, d_conic, dd = d_mean + ed["dL_dmean2D"], d_conic + ed["dL_dconic"], ed["dL_dcolor"][:, 0]
    co = g["conicOpacity"].astype(np.float64)
    K = np.stack([np.stack([co[:, 0], co[:, 1]], 1), np.stack([co[:, 1], co[:, 2]], 1)], 1)
    gK = np.stack([np.stack([d_conic[:, 0], 0.5 * d_conic[:, 1]], 1), np.stack([0.5 * d_conic[:, 1], d_conic[:, 2]], 1)], 1)
    gM = -K @ gK @ K
    grads = {"dL_dmean2D": d_mean, "dL_dcov2D": np.stack([gM[:, 0, 0], gM[:, 0, 1], gM[:, 1, 1]], 1), "dL_ddepths": dd,
             "dL_dcolors": e["dL_dcolor"]}
    sh_degree = 3 if profile == "inria" else 0
    args, kw = _camera_reference(r, cam, grads, f["clamped"], profile, mode, sh_degree)
    exp, M = camera_grad(*args, **kw)
    scale = float(np.abs(exp).max())
    err = float(np.abs(got - exp).max())
    assert scale > 0 and err <= 2e-4 * scale, f"{profile}/{mode}: max abs err {err} at scale {scale}"
    args_t, _ = _camera_reference(r, cam, grads, f["clamped"], profile, mode, sh_degree, view=with_transposed_rotation(cam).view)
    assert float(np.abs(camera_grad(*args_t, **kw)[0] - exp).max()) > 10 * 2e-4 * scale      # the guard


# ---- e. the frustum clamp ------------------------------------------------------------------------------------------------
CLAMP_GROUPS = ("x beyond +1.3 tan", "x beyond -1.3 tan", "y beyond 1.3 tan", "x and y beyond", "off screen, not clamped")


def _clamp_scene(profile, cam):
    """600 Gaussians of the garden-like scene plus five groups of eight large, faint ones placed in view space (ids 600 ..
    639): |t.x / t.z| (|t.y / t.z|) beyond 1.3 tan_fov for the clamped groups, between 1.0 and 1.2 tan_fov — off screen,
    inside the limit — for the last. Nearly round, with scales of 1.8 to 2.2 times the centre's distance from the
    screen edge: the frame lies well inside their 3 sigma, and their extent along the viewing direction — through which
    alone t.x and t.y move cov2D — is as large as across it.
    upstream profile: the clamped ratios lie between 1.4 and 2.5 tan_fov, at t.z of 2.5 to 4.
    gscuda profile: its forward culls a Gaussian whose projected centre x / (w + 0.001) lies beyond +-1.3 in NDC before it
    computes a covariance (csrc/preprocess.hip, in_frustum; GSCuda.cu), so at 1.4 tan_fov nothing is visible under it. A
    Gaussian is visible AND clamped only where the 0.001 in that quotient holds the NDC coordinate inside while the ratio
    is outside: 1.3 < |ratio| / tan_fov < 1.3 (1 + 0.001 / t.z). The groups are placed in that window, at t.z of 0.22 to
    0.3 (the near cull is t.z <= 0.2), 1.3e-3 to 0.8e-3 / t.z beyond the limit — the only clamped Gaussians the profile's
    backward can meet. Returns (scene, ids [5][8])."""
    from helpers import world_from_view
    n0 = 600
    base = _scene(profile, n0, seed=9)
    rng = np.random.default_rng(31)
    tx_, ty_ = cam.tan_fovx, cam.tan_fovy
    window = profile != "inria"
    z = rng.uniform(0.22, 0.3, 40) if window else rng.uniform(2.5, 4.0, 40)
    z[32:] = rng.uniform(2.5, 4.0, 8)
    ratios = []
    for grp in range(5):
        for j in range(8):
            zj = z[8 * grp + j]
            beyond = lambda: 1.3 * (1.0 + rng.uniform(1.3e-3, 0.8e-3 / zj)) if window else rng.uniform(1.4, 2.5)
            sign = lambda: rng.choice([-1.0, 1.0])
            in_ = rng.uniform(-0.6, 0.6)
            rx, ry = (lambda: (beyond(), in_), lambda: (-beyond(), in_), lambda: (in_, beyond() * sign()),
                      lambda: (beyond() * sign(), beyond() * sign()), lambda: (rng.uniform(1.0, 1.2) * sign(), in_))[grp]()
            ratios.append((rx * tx_, ry * ty_))
    ratios = np.asarray(ratios)
    t = np.stack([ratios[:, 0] * z, ratios[:, 1] * z, z], 1)
    extra = {k: np.zeros((40,) + v.shape[1:], v.dtype) for k, v in base.items()}
    extra["means3D"][:, :3] = world_from_view(cam, t)
    extra["means3D"][:, 3] = 1.0
    beyond = np.maximum(np.abs(ratios[:, 0]) - tx_, np.abs(ratios[:, 1]) - ty_).clip(0.1 * ty_) * z   # world distance to the frustum's side
    extra["scales"][:, :3] = (beyond[:, None] * rng.uniform(1.8, 2.2, (40, 3))).astype(np.float32)
    extra["scales"][:, 3] = np.e
    q = rng.normal(size=(40, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    extra["rotations"][:] = q * (rng.uniform(0.8, 1.25, (40, 1)) if profile == "inria" else 1.0)
    extra["opacities"][:] = rng.uniform(0.05, 0.15, 40)
    extra["shs"][:] = rng.normal(0, 0.35, (40, 48))
    extra["shs"][:, :3] += 2.0                               # brighter than what lies behind them (see the test's dL)
    if profile != "inria":
        extra["shs"][:, 3:] = 0.0
    scene = {k: np.ascontiguousarray(np.concatenate([base[k], extra[k]], 0)) for k in base}
    return scene, (n0 + np.arange(40)).reshape(5, 8)


def _clamp_ratios_f32(cam, means):
    """t.x / t.z and t.y / t.z in float32 in the kernels' operation order, and the limits 1.3f tan_fov."""
    f = np.float32
    v = np.asarray(cam.view, f)
    m = np.asarray(means, f)
    one = f(1.0)
    tx = (v[0] * m[:, 0] + v[4] * m[:, 1]) + (v[8] * m[:, 2] + v[12] * one)
    ty = (v[1] * m[:, 0] + v[5] * m[:, 1]) + (v[9] * m[:, 2] + v[13] * one)
    tz = (v[2] * m[:, 0] + v[6] * m[:, 1]) + (v[10] * m[:, 2] + v[14] * one)
    return tx / tz, ty / tz, f(1.3) * f(cam.tan_fovx), f(1.3) * f(cam.tan_fovy)


@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_frustum_clamp_under_a_rotated_pose(profile):
    """clx / cly of both kernels: a clamped ratio passes its gradient to t.z alone. The placed Gaussians are asserted to be
    visible, and on the intended side of the limit by 1e-3 at least in the kernels' float32 arithmetic (so that the float32
    and float64 decisions agree); the chain is checked for exactly these, the camera gradient for the frame. Guard: the
    oracle without the clamp (limits 1e9) must differ on every visible Gaussian of the clamped groups."""
    import torch
    from helpers import chain_seen
    cam = _camera("P1")
    scene, groups = _clamp_scene(profile, cam)
    n = scene["means3D"].shape[0]
    rx, ry, limx, limy = _clamp_ratios_f32(cam, scene["means3D"][groups.reshape(-1)])
    rx, ry = rx.reshape(5, 8), ry.reshape(5, 8)
    over = lambda v, lim: np.abs(v) > lim * (1 + 1e-3)
    under = lambda v, lim: np.abs(v) < lim * (1 - 1e-3)
    assert (over(rx[0], limx) & (rx[0] > 0) & under(ry[0], limy)).all()
    assert (over(rx[1], limx) & (rx[1] < 0) & under(ry[1], limy)).all()
    assert (under(rx[2], limx) & over(ry[2], limy)).all()
    assert (over(rx[3], limx) & over(ry[3], limy)).all()
    assert (under(rx[4], limx) & under(ry[4], limy)).all() and (np.abs(rx[4]) > np.float32(cam.tan_fovx)).all()
    r = _rasterizer(scene, cam)
    kw = _kw(profile)
    r.draw(cam, plan="sort", tile_history=False, **kw)
    g, _, _, clamped = _state(r)
    _assert_seen_enough(np.nonzero(g["radii"][:600] > 0)[0], 600, r)
    shown = g["radii"][groups] > 0
    assert (shown.sum(1) >= 4).all(), shown.sum(1)          # every branch is reached by visible Gaussians
    # dL_dout of one sign over Gaussians brighter than what lies behind them: every pixel then pulls a placed Gaussian's
    # covariance the same way, and the term the clamp reroutes is 40 to 160 times the tolerance on each of them (measured
    # on the float64 reference alone, three noise seeds); under white noise it cancels to below 10 on one or two of the 32
    rng = np.random.default_rng(37)
    dL = (1.0 + 0.25 * rng.normal(size=(3, H, W))).astype(np.float32)
    gd = rng.normal(size=(H, W)).astype(np.float32)
    out = _numpy(r.backward(torch.from_numpy(dL), dL_ddepth=torch.from_numpy(gd), depth="inverse", wide_sums=True, camera=True,
                            **kw))
    ids = groups.reshape(-1)
    chain = dict(out)
    chain["dL_dmeans3D"] = out["dL_dmeans3D"].copy()
    chain["dL_dmeans3D"][:, :3] -= depth_mean_term(scene["means3D"][:, :3], np.asarray(cam.view, np.float32), out["dL_ddepths"], True)
    e = _expected_chain(profile, chain, g, scene, cam, ids, clamped)
    mags = _check_chain(profile, chain, g, scene, cam, ids, clamped, expected=e)
    assert all(m > 0 for m in mags)
    got_upstream = np.abs(out["dL_dcov2D"][groups]).max(2) > 0
    assert ((shown & got_upstream).sum(1) >= 4).all(), (shown & got_upstream).sum(1)     # ... that carry gradient
    faulted = _expected_chain(profile, chain, g, scene, cam, ids, clamped, no_clamp=True)
    seen = chain_seen(e, faulted).reshape(5, 8)
    live = shown & got_upstream
    assert (seen[:4] | ~live[:4]).all(), f"{profile}: without the clamp the reference is the same for {np.nonzero(~seen[:4] & live[:4])}"
    assert not seen[4].any()                                # (and nothing changes for those inside the limit)
    _check_camera(r, cam, out, clamped, profile, "inverse", f"{profile}: frame with clamped Gaussians")


# ---- f. scale_modifier ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0.5, 2.0])
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_scale_modifier_in_the_backward(profile, m):
    """scale_modifier enters dL_dscales twice — as mod s inside M = R diag(mod s), and as the outer factor — and
    dL_drotations through M. draw() and backward() with m at P1, the chain against the oracle with m. Guard: the oracle with
    scale_modifier = 1."""
    import torch
    from helpers import chain_seen
    from oracle import backward_np as B
    n = 600
    scene = _scene(profile, n, seed=6)
    cam = _camera("P1")
    r = _rasterizer(scene, cam)
    kw = _kw(profile)
    r.draw(cam, plan="sort", tile_history=False, scale_modifier=m, **kw)
    g, _, _, clamped = _state(r)
    vis = np.nonzero(g["radii"] > 0)[0]
    _assert_seen_enough(vis, n, r)
    # the factor reached the forward: cov3D is that of M = R diag(m s)
    cov3d = B.inria_cov3d if profile == "inria" else B.cov3d
    for i in vis[:20]:
        c = cov3d(scene["scales"][i, :3], scene["rotations"][i], m)
        assert np.abs(g["cov3D"][i] - c).max() <= 1e-5 * np.abs(c).max(), i
        assert np.abs(g["cov3D"][i] - cov3d(scene["scales"][i, :3], scene["rotations"][i], 1.0)).max() > 0.1 * np.abs(c).max()
    dL = np.random.default_rng(41).normal(size=(3, H, W)).astype(np.float32)
    got = _numpy(r.backward(torch.from_numpy(dL), wide_sums=True, scale_modifier=m, **kw))
    e = _expected_chain(profile, got, g, scene, cam, vis, clamped, scale_modifier=m)
    mags = _check_chain(profile, got, g, scene, cam, vis, clamped, scale_modifier=m, expected=e)
    assert all(v > 0 for v in mags)
    _assert_culled_zero(profile, got, g)
    faulted = _expected_chain(profile, got, g, scene, cam, vis, clamped, scale_modifier=1.0)
    for k in ("dL_dscales", "dL_drotations"):
        _guard_share(chain_seen({k: e[k]}, {k: faulted[k]}), f"{profile}/m={m}: {k}")


# ---- g. the SH gradient's tails (upstream profile) -----------------------------------------------------------------------
def _sh_case(scene, cam, deg, nan_fill=False):
    import torch
    r = _rasterizer(scene, cam)
    kw = _kw("inria", deg)
    r.draw(cam, plan="sort", tile_history=False, **kw)
    g, _, _, clamped = _state(r)
    dL = torch.from_numpy(np.random.default_rng(43).normal(size=(3, cam.height, cam.width)).astype(np.float32))
    out = r.backward(dL, wide_sums=True, **kw)
    if nan_fill:
        # the buffers are this object's and reused by the next call: a row the kernel does not write keeps the NaN
        for k in ("dL_dshs", "dL_dmeans3D"):
            out[k].fill_(float("nan"))
        out = r.backward(dL, wide_sums=True, **kw)
    return r, g, clamped, _numpy(out)


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257])
def test_sh_gradient_tails(n, deg):
    """The upstream chain stages 64 x 48 SH floats per wave through LDS in 16-byte pieces, with a tail test against 48 n and
    a number of pieces that depends on the degree: n around the wave and block sizes x every degree, on 64 x 48 at P1.
    dL_dshs and dL_dmeans3D (and the rest of the chain) per Gaussian; nothing beyond 3 (deg + 1)^2."""
    cam = _camera("P1", 64, 48)
    scene = _scene("inria", n, seed=50 + n)
    scene["opacities"] = np.maximum(scene["opacities"], np.float32(0.3))       # (n = 1: the one Gaussian must be composited)
    scene["scales"][:, :3] = np.maximum(scene["scales"][:, :3], np.float32(0.03))
    r, g, clamped, got = _sh_case(scene, cam, deg)
    vis = np.nonzero(g["radii"] > 0)[0]
    _assert_seen_enough(vis, n, r)
    mags = _check_chain("inria", got, g, scene, cam, vis, clamped, deg=deg)
    assert mags[1] > 0 and mags[4] > 0
    _assert_culled_zero("inria", got, g)
    assert got["dL_dshs"].shape == (n, 48) and (got["dL_dshs"][:, 3 * (deg + 1) ** 2:] == 0).all()
    assert np.isfinite(got["dL_dshs"]).all()


def test_sh_gradient_of_a_wholly_culled_wave():
    """n = 320 with Gaussians 64 .. 127 — one whole wave: the __ballot(visible) skip — and 250 .. 255 behind the camera.
    dL_dshs is filled with NaN before the call: the culled rows must come back as exact zeros, their neighbours right."""
    from helpers import view_from_world, world_from_view
    cam = _camera("P1", 64, 48)
    n = 320
    scene = _scene("inria", n, seed=61)
    behind = np.concatenate([np.arange(64, 128), np.arange(250, 256)])
    rng = np.random.default_rng(62)
    t = np.stack([rng.uniform(-1, 1, behind.size), rng.uniform(-1, 1, behind.size), -rng.uniform(0.5, 3.0, behind.size)], 1)
    scene["means3D"][behind, :3] = world_from_view(cam, t)
    assert (view_from_world(cam, scene["means3D"][behind, :3])[:, 2] < -0.4).all()
    r, g, clamped, got = _sh_case(scene, cam, 3, nan_fill=True)
    assert (g["radii"][behind] == 0).all()                  # the culled wave is there
    vis = np.nonzero(g["radii"] > 0)[0]
    _assert_seen_enough(vis, n - behind.size, r)
    for lo, hi in ((56, 64), (128, 136), (244, 250), (256, 262)):
        assert (g["radii"][lo:hi] > 0).sum() >= 2, (lo, hi)  # visible neighbours on both sides
    assert np.isfinite(got["dL_dshs"]).all() and np.isfinite(got["dL_dmeans3D"]).all()
    assert (got["dL_dshs"][behind] == 0).all() and (got["dL_dmeans3D"][behind] == 0).all()
    mags = _check_chain("inria", got, g, scene, cam, vis, clamped, deg=3)
    assert mags[4] > 0
    _assert_culled_zero("inria", got, g)
