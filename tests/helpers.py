"""Shared helpers for the parity tests."""
import os

import numpy as np

from gsrast_amd.camera import Camera

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INT_KEYS = ["radii", "tilesTouched", "pointOffsets", "rects", "keys_unsorted", "values_unsorted", "keys", "values",
            "ranges", "nContrib"]
FLT_KEYS = ["means2D", "depths", "cov3D", "rgb", "conicOpacity", "finalT", "out_color"]


def load_golden(name="config1.npz"):
    z = np.load(os.path.join(ROOT, "tests", "golden", name))
    n = z["in_means3D"].shape[0]
    shs = np.zeros((n, 48), np.float32)
    shs[:, :3] = z["in_shs_dc"]
    scene = {"means3D": z["in_means3D"], "scales": z["in_scales"], "rotations": z["in_rotations"],
             "opacities": z["in_opacities"], "shs": shs}
    cam = Camera(view=z["cam_view"], proj=z["cam_proj"], cam_pos=z["cam_pos"], tan_fovx=float(z["cam_tan"][0]),
                 tan_fovy=float(z["cam_tan"][1]), width=int(z["size"][0]), height=int(z["size"][1]))
    exp = {k[4:]: z[k] for k in z.files if k.startswith("exp_")}
    exp["num_rendered"] = int(z["num_rendered"])
    exp["records_staged"] = int(z["records_staged"])
    return scene, cam, tuple(float(v) for v in z["background"]), exp


def single_gaussian_scene(pos=(0.0, 0.0, 0.0), scale=0.1, opacity=0.8, dc=(1.0, 0.5, -0.5), quat=(1, 0, 0, 0), n=1):
    """n copies of one isotropic Gaussian (positions may be overridden by the caller)."""
    means = np.ones((n, 4), np.float32)
    means[:, :3] = np.asarray(pos, np.float32)
    scales = np.full((n, 4), np.e, np.float32)
    scales[:, :3] = scale
    rot = np.tile(np.asarray(quat, np.float32), (n, 1))
    shs = np.zeros((n, 48), np.float32)
    shs[:, :3] = np.asarray(dc, np.float32)
    return {"means3D": means, "scales": scales, "rotations": rot,
            "opacities": np.full(n, opacity, np.float32), "shs": shs}


def image_report(got, exp, tol=1e-4):
    """Max abs error plus the pixels over tolerance (threshold-flip candidates)."""
    d = np.abs(got.astype(np.float64) - exp.astype(np.float64))
    per_pixel = d.max(axis=0) if d.ndim == 3 else d
    bad = per_pixel > tol
    return float(d.max()), int(bad.sum()), per_pixel


PIXEL_TOL = 2e-6     # measured 3.6e-7: the colour sums are three fused multiply-adds on alpha T where the reference rounds twice


def assert_blend_parity(img, final_t, n_contrib, exp, what="", bitwise_t=True):
    """The tile loop's outputs against the oracle's. The HIP blend evaluates power, the exponential (as glibc's expf: the
    oracle's), alpha, T and every test in the reference's float32 operation order, so the transmittance and the last
    contributor are the oracle's BIT FOR BIT — no pixel sits on the other side of a threshold — and the colours differ by the
    rounding of the fused sums only: far inside the north star's 1e-4. bitwise_t=False: `exp` comes from the committed fixture,
    minted by the numpy restatement (whose float32 exp is not libm's): transmittance within 1e-6 then."""
    nc = np.asarray(n_contrib).view(np.uint32)
    flips = int((nc != exp["nContrib"]).sum())
    ft = np.asarray(final_t)
    t_diff = int((ft.view(np.uint32) != exp["finalT"].view(np.uint32)).sum())
    max_err, n_bad, _ = image_report(np.asarray(img), exp["out_color"], 1e-4)
    print(f"[parity] {what}: max abs pixel err {max_err:.3e}, pixels > 1e-4: {n_bad}, finalT words differing: {t_diff}, nContrib flips: {flips}")
    assert flips == 0 and (t_diff == 0 if bitwise_t else float(np.abs(ft - exp["finalT"]).max()) <= 1e-6), (what, flips, t_diff)
    assert n_bad == 0 and max_err <= PIXEL_TOL, (what, max_err, n_bad)
    return max_err


def _rotate_about(v, axis, angle):
    """Rodrigues: v turned by `angle` about the unit vector `axis` (float64)."""
    v, k = np.asarray(v, np.float64), np.asarray(axis, np.float64)
    return v * np.cos(angle) + np.cross(k, v) * np.sin(angle) + k * (k @ v) * (1.0 - np.cos(angle))


def posed_camera(w, h, eye, target=(0.0, 0.0, 0.0), roll=0.0, kx=1.0, near=0.05, far=50.0):
    """A camera at `eye` looking at `target`, rolled by `roll` about its viewing direction, prepared as
    camera.first_person_camera prepares its arguments: proj = perspective . view in float32, then row 2 of the view matrix
    negated, both column-major. The up vector is (0, -1, 0) turned by `roll` about the viewing direction. kx: non-square
    pixels as in test_non_square_pixels_use_both_focal_lengths — tan_fovx = kx tan_fovy W / H with the matching projection,
    so focal_x / focal_y = 1 / kx. The rotation block of the view matrix must not be symmetric (max |R - R^T| > 0.1):
    under a symmetric one a transposed index in the backward chain changes nothing, and a test through this camera is blind."""
    import math
    from gsrast_amd import camera
    F = np.float32
    fov = math.radians(45.0)
    eye = np.asarray(eye, F).reshape(3)
    target = np.broadcast_to(np.asarray(target, F), (3,))
    front = (target - eye).astype(np.float64)
    front /= np.linalg.norm(front)
    up = _rotate_about((0.0, -1.0, 0.0), front, roll).astype(F)
    view = camera.look_at(eye, target, up)
    aspect = F(w) / F(h) * F(kx)
    proj = (camera.perspective(fov, aspect, near, far) @ view).astype(F)
    view = view.copy()
    view[2, :] *= F(-1.0)
    tan_y = float(F(math.tan(F(fov) * F(0.5))))
    cam = Camera(view=np.ascontiguousarray(view.T).reshape(16).copy(), proj=np.ascontiguousarray(proj.T).reshape(16).copy(),
                 cam_pos=eye.copy(), tan_fovx=float(F(tan_y) * aspect), tan_fovy=tan_y, width=w, height=h)
    R = view[:3, :3].astype(np.float64)
    assert np.abs(R - R.T).max() > 0.1, ("the pose's rotation block is (nearly) symmetric", R)
    return cam


def view_rotation(cam):
    """The rotation block R of cam.view (t = R m + T), float64 [3,3]."""
    return np.asarray(cam.view, np.float64).reshape(4, 4).T[:3, :3].copy()


def view_from_world(cam, m):
    """t = V (m, 1) in float64: the view-space position computeCov2D clamps. m [n,3] -> [n,3]."""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    return np.asarray(m, np.float64).reshape(-1, 3) @ V[:3, :3].T + V[:3, 3]


def world_from_view(cam, t):
    """The world positions [n,3] (float64) whose view-space positions under cam.view are t [n,3]: scenes placed relative to
    the frustum of a rotated camera."""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    return np.linalg.solve(V[:3, :3], (np.asarray(t, np.float64).reshape(-1, 3) - V[:3, 3]).T).T


def with_transposed_rotation(cam):
    """cam with the rotation block of its view matrix transposed: the reference input of a fault that indexes the view
    matrix the wrong way round (blindness guards)."""
    import dataclasses
    V = np.asarray(cam.view, np.float32).reshape(4, 4).T.copy()
    V[:3, :3] = V[:3, :3].T.copy()
    return dataclasses.replace(cam, view=np.ascontiguousarray(V.T).reshape(16).copy())


def _rows_differ(e, f, tol):
    """Per row: does f differ from e by more than tol of the row's own largest component (floored as the chain checks
    floor it, at 1e-3 of the largest over all rows)?"""
    if len(e) == 0:
        return np.zeros(0, bool)
    mag = np.maximum(np.abs(e).max(1), 1e-3 * np.abs(e).max())
    return np.abs(f - e).max(1) > tol * np.maximum(mag, 1e-30)


CHAIN_TOL = {"dL_dcov3D": 2e-3, "dL_dmeans3D": 3e-3, "dL_dscales": 3e-3, "dL_drotations": 3e-3, "dL_dshs": 1e-4}


def chain_seen(exp, faulted, factor=10.0, tol_scale=1.0):
    """bool[len(ids)]: the Gaussians on which a reference computed from faulted inputs (`faulted`, keyed like `exp`: the
    dicts of backward_chain_expected*) differs from the true one by more than `factor` times the chain check's tolerance in
    some array, measured on the Gaussian's own largest component — where the chain check would see that fault."""
    seen = None
    for k, e in exp.items():
        d = _rows_differ(e, faulted[k], factor * CHAIN_TOL[k] * tol_scale)
        seen = d if seen is None else (seen | d)
    return seen


def backward_chain_expected(got, g, scene, cam, w, h, ids, upstream=None, scale_modifier=1.0, no_clamp=False):
    """The float64 expectation of check_backward_chain: dict dL_dcov3D [m,6], dL_dmeans3D [m,3], dL_dscales [m,3],
    dL_drotations [m,4] for the Gaussians `ids`. no_clamp: the +-1.3 tan(fov) limits replaced by 1e9 (blindness guards)."""
    from oracle import backward_np as B
    focal = h / (2.0 * cam.tan_fovy)
    tanx, tany = (1e9, 1e9) if no_clamp else (cam.tan_fovx, cam.tan_fovy)
    m = len(ids)
    exp_cov, exp_mean, exp_scale, exp_rot = np.zeros((m, 6)), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 4))
    for j, i in enumerate(ids):
        c3 = g["cov3D"][i].astype(np.float64)
        m3 = scene["means3D"][i, :3].astype(np.float64)
        up = got if upstream is None else upstream
        dconic = up["dL_dconic_opacity"][i, :3].astype(np.float64)
        # (the chain starts from the summed dL/dcov2D where the call produced it: gsr_backward_args.dL_dcov2D)
        dcov = up["dL_dcov2D"][i].astype(np.float64) if "dL_dcov2D" in up else None
        exp_cov[j] = B.conic_backward(c3, m3, cam.view, focal, tanx, tany, dconic, dcov)
        exp_mean[j] = (B.project_mean2d_backward(m3, cam.proj, w, h, up["dL_dmean2D"][i].astype(np.float64)) +
                       B.conic_backward_mean(c3, m3, cam.view, focal, tanx, tany, dconic, dcov))
        exp_scale[j], exp_rot[j] = B.cov3d_backward(scene["scales"][i, :3], scene["rotations"][i], scale_modifier,
                                                    (got["dL_dcov3D"][i] if upstream is None else exp_cov[j]).astype(np.float64))
    return {"dL_dcov3D": exp_cov, "dL_dmeans3D": exp_mean, "dL_dscales": exp_scale, "dL_drotations": exp_rot}


def check_backward_chain(got, g, scene, cam, w, h, ids, upstream=None, tol_scale=1.0, scale_modifier=1.0, expected=None):
    """gsr_backward's per-Gaussian chain (cov2D -> cov3D -> scales / rotations, pixel centre and Jacobian -> means3D)
    for the Gaussians `ids`, against oracle/backward_np.py fed with the GPU's own upstream gradients — or, with `upstream`
    (dict: dL_dmean2D, dL_dconic_opacity, dL_dcov2D indexable like `got`), with sums computed independently of the GPU: an
    end-to-end check. `got`: the gradient arrays (numpy, full size or indexable by id), `g`: geometry state arrays (cov3D),
    `scene`: host inputs. scale_modifier: that of the draw() and backward() calls. expected: the result of
    backward_chain_expected for the same arguments, where the caller has it already. Returns the largest expected magnitude
    of (dL_dcov3D, dL_dmeans3D, dL_dscales, dL_drotations)."""
    m = len(ids)
    exp = expected if expected is not None else backward_chain_expected(got, g, scene, cam, w, h, ids, upstream, scale_modifier)
    exp_cov, exp_mean, exp_scale, exp_rot = (exp[k] for k in ("dL_dcov3D", "dL_dmeans3D", "dL_dscales", "dL_drotations"))
    ids = np.asarray(ids)
    # compared per Gaussian relative to its own magnitude (float32 outputs of a chain evaluated in double). End to end
    # (`upstream`): the rotation gradient of a nearly round splat is a difference of nearly equal products — it vanishes for a
    # round one — so that what is left of the sums' sixth digit shows in its third: ten times the tolerance of the others.
    for name, e, gotv, tol in (("dL_dcov3D", exp_cov, got["dL_dcov3D"][ids], 2e-3),
                               ("dL_dmeans3D", exp_mean, got["dL_dmeans3D"][ids][:, :3], 3e-3),
                               ("dL_dscales", exp_scale, got["dL_dscales"][ids][:, :3], 3e-3),
                               ("dL_drotations", exp_rot, got["dL_drotations"][ids], 3e-3 if upstream is None else 3e-2)):
        if m == 0:
            continue
        err = np.abs(gotv - e).max(1)
        mag = np.maximum(np.abs(e).max(1), 1e-3 * np.abs(e).max())
        if upstream is not None:
            print(f"[backward] end to end, {name}: worst error {float((err / np.maximum(mag, 1e-30)).max()):.2e} of the Gaussian's own largest component")
        assert (err <= tol * tol_scale * np.maximum(mag, 1e-30)).all(), (name, float((err / np.maximum(mag, 1e-30)).max()))
    return [float(np.abs(e).max()) if m else 0.0 for e in (exp_cov, exp_mean, exp_scale, exp_rot)]


def backward_chain_expected_inria(got, g, scene, cam, w, h, ids, deg, clamped, upstream=None, scale_modifier=1.0,
                                  no_clamp=False, swap_focal=False):
    """The float64 expectation of check_backward_chain_inria: dict dL_dcov3D, dL_dmeans3D, dL_dscales, dL_drotations,
    dL_dshs [m,48]. no_clamp / swap_focal: faulted reference inputs (blindness guards) — the +-1.3 tan(fov) limits replaced
    by 1e9; focal_x and focal_y exchanged."""
    from oracle import backward_np as B
    fx, fy = w / (2.0 * cam.tan_fovx), h / (2.0 * cam.tan_fovy)
    if swap_focal:
        fx, fy = fy, fx
    tanx, tany = (1e9, 1e9) if no_clamp else (cam.tan_fovx, cam.tan_fovy)
    m = len(ids)
    exp_cov, exp_mean, exp_scale, exp_rot, exp_sh = np.zeros((m, 6)), np.zeros((m, 3)), np.zeros((m, 3)), np.zeros((m, 4)), np.zeros((m, 48))
    up = got if upstream is None else upstream
    for j, i in enumerate(ids):
        c3 = g["cov3D"][i].astype(np.float64)
        m3 = scene["means3D"][i, :3].astype(np.float64)
        dconic = up["dL_dconic_opacity"][i, :3].astype(np.float64)
        dcov = up["dL_dcov2D"][i].astype(np.float64) if "dL_dcov2D" in up else None
        exp_cov[j], g_mean_j = B.inria_conic_backward(c3, m3, cam.view, fx, fy, tanx, tany, dconic, dcov)
        g_sh, g_mean_c = B.inria_color_backward(m3, cam.cam_pos, scene["shs"][i].reshape(16, 3), deg, up["dL_dcolors"][i].astype(np.float64))
        # the oracle decides the clamp from its own float64 colour; the kernel uses the forward's flags: they must agree
        raw_negative = B.inria_color(m3, cam.cam_pos, scene["shs"][i].reshape(16, 3), deg) == 0.0
        assert (raw_negative == clamped[i]).all() or np.abs(g["rgb"][i]).min() < 1e-6
        exp_sh[j] = g_sh.reshape(48)
        exp_mean[j] = (B.inria_project_mean2d_backward(m3, cam.proj, w, h, up["dL_dmean2D"][i].astype(np.float64)) + g_mean_j + g_mean_c)
        exp_scale[j], exp_rot[j] = B.inria_cov3d_backward(scene["scales"][i, :3], scene["rotations"][i], scale_modifier,
                                                          (got["dL_dcov3D"][i] if upstream is None else exp_cov[j]).astype(np.float64))
    return {"dL_dcov3D": exp_cov, "dL_dmeans3D": exp_mean, "dL_dscales": exp_scale, "dL_drotations": exp_rot, "dL_dshs": exp_sh}


def check_backward_chain_inria(got, g, scene, cam, w, h, ids, deg, clamped, upstream=None, scale_modifier=1.0, expected=None):
    """The upstream profile's per-Gaussian chain for the Gaussians `ids` against oracle/backward_np.py (inria_*), fed with
    the GPU's own upstream gradients — or, with `upstream` (dict: dL_dmean2D, dL_dconic_opacity, dL_dcolors and optionally
    dL_dcov2D, indexable like `got`), with sums computed independently of the GPU: end to end, under check_backward_chain's
    tolerances for that case (the rotation gradient at ten times the others': see there; the SH gradient is B_k times the
    colour sums, which the callers compare with the blend reference themselves: not repeated end to end). clamped: bool[N,3] of the forward call. scale_modifier: that of the draw() and
    backward() calls. expected: the result of backward_chain_expected_inria for the same arguments, where the caller has
    it already. Returns the largest expected magnitudes of (dL_dcov3D, dL_dmeans3D, dL_dscales, dL_drotations, dL_dshs)."""
    m = len(ids)
    exp = expected if expected is not None else backward_chain_expected_inria(got, g, scene, cam, w, h, ids, deg, clamped, upstream,
                                                                              scale_modifier)
    exp_cov, exp_mean, exp_scale, exp_rot, exp_sh = (exp[k] for k in ("dL_dcov3D", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dshs"))
    ids = np.asarray(ids)
    for name, e, gotv, tol in (("dL_dcov3D", exp_cov, got["dL_dcov3D"][ids], 2e-3),
                               ("dL_dmeans3D", exp_mean, got["dL_dmeans3D"][ids][:, :3], 3e-3),
                               ("dL_dscales", exp_scale, got["dL_dscales"][ids][:, :3], 3e-3),
                               ("dL_drotations", exp_rot, got["dL_drotations"][ids], 3e-3 if upstream is None else 3e-2),
                               ("dL_dshs", exp_sh, got["dL_dshs"][ids], 1e-4)):
        if m == 0 or (upstream is not None and name == "dL_dshs"):
            continue
        err = np.abs(gotv - e).max(1)
        mag = np.maximum(np.abs(e).max(1), 1e-3 * np.abs(e).max())
        if upstream is not None:
            print(f"[backward] end to end (upstream profile), {name}: worst error {float((err / np.maximum(mag, 1e-30)).max()):.2e} of the Gaussian's own largest component")
        assert (err <= tol * np.maximum(mag, 1e-30)).all(), (name, float((err / np.maximum(mag, 1e-30)).max()))
    return [float(np.abs(e).max()) if m else 0.0 for e in (exp_cov, exp_mean, exp_scale, exp_rot, exp_sh)]


_GRAD_KEYS = (("dL_dmean2D", "d_mean", "M_mean"), ("dL_dconic", "d_conic", "M_conic"), ("dL_dcov2D", "d_cov", "M_cov"),
              ("dL_dopacity", "d_op", "M_op"), ("dL_dcolors", "d_col", "M_col"))


def oracle_gradients(r, dL, bg, tiles, targets, max_depth, bad_pixels=None, f32_forward=False, magnitudes=False, t_cutoff=0.001,
                     full_lists=False):
    """Float64 gradients (oracle/backward_np.blend_tile_backward) of the Gaussians `targets`, summed over `tiles` (which must
    contain every tile those Gaussians touch), from the forward state of the rasterizer `r` (its means2D, conics, colours and
    sorted lists). Returns a dict:
      exp      {dL_dmean2D [n,2], dL_dconic [n,3], dL_dcov2D [n,3], dL_dopacity [n,1], dL_dcolors [n,3]}
      differs  (y, x) of every pixel whose last contributor differs from the GPU's nContrib
    and with magnitudes=True also
      M        the condition scale of every sum, keyed like exp (blend_tile_backward's M_*)
      k        [n] walk depth (largest over the Gaussian's records); pixels, free_pixels [n]: contributing pixels, and those of
               them where alpha is not clamped; tiles [n]: tiles where the Gaussian contributes
      n_contrib, final_t  the oracle's per-pixel outputs [H,W] on the evaluated tiles (elsewhere -1 and NaN), stop_idx [H,W]
    bad_pixels (a list, optional): receives (y, x) of every pixel on which the oracle's forward and the GPU's disagree —
    another last contributor, or another transmittance (a record at alpha = 1/255 taken by one of them only).
    full_lists: evaluate every tile's whole list (else the prefix that reaches the GPU's deepest last contributor of the tile:
    enough when the GPU's nContrib is right, which the caller must then check on its own)."""
    import torch
    from oracle import backward_np as B
    W, H = r.width, r.height
    gx = (W + 15) // 16
    geo = r.map_geometry_state()
    ranges = r.map_image_state()["ranges"].cpu().numpy().view(np.uint32).astype(np.int64)
    ncontrib = r.map_image_state()["nContrib"]
    plist = r.map_binning_state()["values"]
    final_t = r.map_image_state()["finalT"]
    row_of = np.full(r.num_gaussians, -1, np.int64)
    row_of[targets] = np.arange(len(targets))
    n = len(targets)
    dims = {"dL_dmean2D": 2, "dL_dconic": 3, "dL_dcov2D": 3, "dL_dopacity": 1, "dL_dcolors": 3}
    sums = {k: np.zeros((n, d)) for k, d in dims.items()}
    mags = {k: np.zeros((n, d)) for k, d in dims.items()}
    k_walk, pixels, free_pixels, n_tiles = (np.zeros(n, np.int64) for _ in range(4))
    nc_frame, ft_frame, stop_frame = np.full((H, W), -1, np.int64), np.full((H, W), np.nan), np.full((H, W), -1, np.int64)
    differs_px = []
    dL_host = dL.cpu().numpy() if hasattr(dL, "cpu") else np.asarray(dL)
    for tx, ty in tiles:
        t = ty * gx + tx
        ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
        nc_tile = ncontrib[ya:yb, xa:xb]
        a = int(ranges[t, 0])
        length = max(0, int(ranges[t, 1]) - a)
        depth = length if full_lists else int(nc_tile.max())     # the list prefix that reaches every pixel's last contributor
        assert depth <= length and depth <= max_depth, (depth, length, max_depth)
        ids = plist[a:a + depth].to(torch.int64)
        tile_g = np.zeros((3, 16, 16))
        tile_g[:, : yb - ya, : xb - xa] = dL_host[:, ya:yb, xa:xb]
        res = B.blend_tile_backward(geo["means2D"][ids].cpu().numpy(), geo["conicOpacity"][ids].cpu().numpy(),
                                    geo["rgb"][ids].cpu().numpy(), tx, ty, W, H, bg, tile_g, t_cutoff=t_cutoff,
                                    f32_forward=f32_forward, magnitudes=magnitudes)
        differs = res["n_contrib"][: yb - ya, : xb - xa] != nc_tile.cpu().numpy()
        bad = int(differs.sum())
        differs_px.extend((ya + int(y), xa + int(x)) for y, x in zip(*np.nonzero(differs)))
        if bad_pixels is not None:
            ft = final_t[ya:yb, xa:xb].cpu().numpy().astype(np.float64)
            differs = differs | (np.abs(res["final_t"][: yb - ya, : xb - xa] - ft) > 1e-5 + 1e-3 * ft)
            bad_pixels.extend((ya + int(y), xa + int(x)) for y, x in zip(*np.nonzero(differs)))
        if bad == 0:       # float32 chain of up to 10 000 records against float64: sanity only (parity is the C++ oracle's job)
            assert np.abs(res["out"][:, : yb - ya, : xb - xa] - r.out_color[:, ya:yb, xa:xb].cpu().numpy()).max() <= 3e-3
        rows = row_of[ids.cpu().numpy()]
        hit = rows >= 0
        for key, d, m in _GRAD_KEYS:
            np.add.at(sums[key], rows[hit], res[d][hit].reshape(-1, sums[key].shape[1]))
            if magnitudes:
                np.add.at(mags[key], rows[hit], res[m][hit].reshape(-1, mags[key].shape[1]))
        if magnitudes:
            np.maximum.at(k_walk, rows[hit], res["k"][hit])
            np.add.at(pixels, rows[hit], res["pixels"][hit])
            np.add.at(free_pixels, rows[hit], res["free_pixels"][hit])
            np.add.at(n_tiles, rows[hit], (res["pixels"][hit] > 0).astype(np.int64))
            nc_frame[ya:yb, xa:xb] = res["n_contrib"][: yb - ya, : xb - xa]
            ft_frame[ya:yb, xa:xb] = res["final_t"][: yb - ya, : xb - xa]
            stop_frame[ya:yb, xa:xb] = res["stop_idx"][: yb - ya, : xb - xa]
    out = {"exp": sums, "differs": differs_px}
    if magnitudes:
        out.update(M=mags, k=k_walk, pixels=pixels, free_pixels=free_pixels, tiles=n_tiles, n_contrib=nc_frame, final_t=ft_frame,
                   stop_idx=stop_frame)
    return out


def gradients_of(got_dev, targets):
    """The render backward's per-Gaussian sums of the Gaussians `targets` (numpy, keyed like oracle_gradients' exp)."""
    import torch
    idx = torch.from_numpy(np.asarray(targets)).to(got_dev["dL_dcolors"].device)
    return {"dL_dmean2D": got_dev["dL_dmean2D"][idx].cpu().numpy(),
            "dL_dconic": got_dev["dL_dconic_opacity"][idx][:, :3].cpu().numpy(),
            "dL_dcov2D": got_dev["dL_dcov2D"][idx][:, :3].cpu().numpy(),
            "dL_dopacity": got_dev["dL_dconic_opacity"][idx][:, 3:4].cpu().numpy(),
            "dL_dcolors": got_dev["dL_dcolors"][idx].cpu().numpy()}


# Per-Gaussian error bound of the render backward (assert_backward_per_gaussian):
#     |got - exp| <= BW_TAU * (k + BW_C [+ tiles with float sums]) * M + BW_ATOL
# M: the sum's condition scale (all factors in absolute value), k: the walk depth (reciprocals behind the rebuilt T), tiles: the
# float sums of the tiles, one per tile in any order (wide_sums=False, or the block feed's per-entry sums). BW_C covers what every record pays whatever its depth: the fused
# sums over a lane's four pixels, the six-level wave reduction, the final rounding. Calibrated on one MI355X over every scene and
# path of tests/test_gpu_backward_edges.py (10 scenes x 6 paths): worst |err| / ((k + 8) M) measured 2.80e-8 (garden pose 1,
# sorted list), 2.54e-8 (garden pose 0), 1.96e-8 (long lists), 1.94e-8 (termination at 1e-4, band), 1.07e-8 (clamp), 9.2e-9
# (screen-filling splat), 6.8e-9 (1/255 twins), 4.5e-9 (per-entry sums scene); with float tile sums worst
# |err| / ((k + 8 + tiles) M) 2.62e-8 (float atomics), 1.47e-9 (per-entry sums). BW_TAU is 4x the worst, just under float32
# epsilon (1.19e-7).
BW_C = 8.0
BW_TAU = 1.1e-7
BW_ATOL = 1e-30


def assert_backward_inputs(n_contrib, final_t, ref, what=""):
    """What the backward reads of the forward — nContrib and finalT — against the float32 oracle's (f32_forward), bit for bit, on
    the pixels the oracle evaluated. A failure here is the FORWARD's (or the oracle's), not the backward's."""
    nc = np.asarray(n_contrib).view(np.uint32).astype(np.int64)
    ft = np.asarray(final_t, np.float32)
    on = ref["n_contrib"] >= 0
    assert on.any(), what
    bad_nc = int((nc[on] != ref["n_contrib"][on]).sum())
    bad_ft = int((ft[on].view(np.uint32) != ref["final_t"][on].astype(np.float32).view(np.uint32)).sum())
    assert bad_nc == 0 and bad_ft == 0, (f"{what}: the forward state differs from the float32 oracle's ({bad_nc} nContrib, {bad_ft} "
                                         "finalT words): the forward (or the oracle's restatement of it) is at fault, not the backward")


def assert_backward_per_gaussian(got, ref, float_tile_sums=False, what=""):
    """The render backward's sums of every Gaussian of `ref` (oracle_gradients(..., f32_forward=True, magnitudes=True)) against
    the oracle's, Gaussian by Gaussian and component by component — not against a scale shared by the whole frame, under which
    the Gaussians behind an opaque front (T ~ 1e-3) could be 100 % wrong:
      support  a Gaussian no pixel composites gets 0.0 in every component, bit for bit; one that some pixel composites gets
               non-zero colour gradients (dL_dout is random: they cannot vanish)
      clamp    a Gaussian clamped (raw > 0.99) on every pixel it composites gets exactly zero mean, conic, opacity and
               covariance gradients
      value    |got - exp| <= BW_TAU (k + BW_C [+ tiles]) M + BW_ATOL
    float_tile_sums: the tiles' sums of a Gaussian were added in float in some order (wide_sums=False, or the block feed's
    per-entry sums): the tiles term is added. got: gradients_of(...). Returns the worst ratio |got - exp| / ((k + BW_C [+ tiles]) M)
    over the components with M > 0 (printed; where M = 0 the bound is BW_ATOL)."""
    exp, M = ref["exp"], ref["M"]
    none = ref["pixels"] == 0
    clamped = (ref["pixels"] > 0) & (ref["free_pixels"] == 0)
    depth = ref["k"].astype(np.float64) + BW_C + (ref["tiles"].astype(np.float64) if float_tile_sums else 0.0)
    worst, worst_at = 0.0, None
    for key, _, _ in _GRAD_KEYS:
        e, m = exp[key], M[key]
        g = np.asarray(got[key], np.float64).reshape(e.shape)
        assert np.isfinite(g).all(), (what, key)
        assert (g[none] == 0.0).all(), (what, key, "a Gaussian no pixel composites must get exactly zero",
                                         np.nonzero(none)[0][(g[none] != 0).any(1)][:8])
        if key != "dL_dcolors":
            assert (g[clamped] == 0.0).all(), (what, key, "a Gaussian clamped on every pixel it composites moves no alpha",
                                               np.nonzero(clamped)[0][(g[clamped] != 0).any(1)][:8])
        err = np.abs(g - e)
        bound = BW_TAU * depth[:, None] * m + BW_ATOL
        ratio = np.where(m > 0, err / np.maximum(depth[:, None] * m, 1e-300), 0.0)
        i = np.unravel_index(int(np.argmax(ratio)), e.shape)
        if ratio[i] > worst:
            worst, worst_at = float(ratio[i]), (key, int(i[0]), int(ref["k"][i[0]]), float(e[i]), float(g[i]), float(m[i]))
        over = err > bound
        assert not over.any(), (what, key, f"{int(over.any(1).sum())} Gaussians over the bound; worst ratio {float(ratio.max()):.3e}",
                                worst_at)
    assert (np.asarray(got["dL_dcolors"])[~none] != 0.0).all(), (what, "a composited Gaussian without colour gradient")
    print(f"[backward per Gaussian] {what}: {int((~none).sum())} composited ({int(clamped.sum())} clamped everywhere), worst "
          f"|err| / ((k + c{' + tiles' if float_tile_sums else ''}) M) = {worst:.3e} at {worst_at}")
    return worst


# ---- the upstream profile (GSR_FLAG_SEMANTICS_INRIA) against its restatement, oracle/inria_np.py ----
def inria_scene(n, seed, sh_scale=0.3, shrink=0.25):
    """The garden-like scene drawn smaller, with all sixteen SH coefficient triples N(0, sh_scale): [N][16][3]."""
    from gsrast_amd import scenes
    sc = scenes.garden_like_scene(n, seed=seed)
    sc["means3D"][:, :3] *= shrink
    sc["shs"] = np.random.default_rng(seed).normal(0, sh_scale, (n, 48)).astype(np.float32)
    return sc


def opaque_stack_scene(n=900, seed=3, spread=1.2):
    """Opaque splats (opacity 0.3 .. 0.99) stacked deep over the middle of the frame, faint ones (1/255 .. 0.05) around them:
    pixels in the middle run into the transmittance cut-off after ten-odd records, those outside walk their lists to the end."""
    rng = np.random.default_rng(seed)
    sc = single_gaussian_scene(n=n)
    sc["means3D"][:, 0] = rng.uniform(-spread, spread, n)
    sc["means3D"][:, 1] = rng.uniform(-spread, spread, n)
    sc["means3D"][:, 2] = rng.uniform(-1.0, 1.0, n)
    sc["scales"][:, :3] = rng.uniform(0.05, 0.3, (n, 3))
    q = rng.normal(0, 1, (n, 4))
    sc["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    inner = np.hypot(sc["means3D"][:, 0], sc["means3D"][:, 1]) < 0.6 * spread
    sc["opacities"] = np.where(inner, rng.uniform(0.3, 0.99, n), rng.uniform(1.0 / 255.0, 0.05, n)).astype(np.float32)
    sc["shs"] = rng.normal(0, 0.3, (n, 48)).astype(np.float32)
    sc["shs"][:, :3] += 1.0
    return sc


def stop_census(exp, cam):
    """Of an inria_np.forward result: how many pixels stop at this profile's cut-off 1e-4, and how many would have stopped at
    the other profile's 1e-3 but do not stop here. A pixel stops at cut-off c exactly if its transmittance, walked to the end
    of its list without any cut-off, falls below c somewhere — it only falls, so: if it ends below c."""
    from oracle import cpu_oracle
    t_end = cpu_oracle.blend_cutoff(exp, cam, threads=4, t_cutoff=0.0)["finalT"]
    return int((t_end < np.float32(1e-4)).sum()), int(((t_end < np.float32(1e-3)) & ~(t_end < np.float32(1e-4))).sum())


def run_inria(scene, cam, bg=(0.0, 0.0, 0.0), **kw):
    """A first draw, every chunk zeroed (so that what a call leaves unwritten compares equal to the restatement's zeros), and
    the draw that is compared, with the staged records counted. Returns (rasterizer, image)."""
    from gsrast_amd.rasterizer import SplatRasterizer
    kw.setdefault("semantics", "inria")
    r = SplatRasterizer(cam.width, cam.height, background=bg)
    r.configure_from_scene(scene)
    r.draw(cam, **kw)
    for cb in (r.geom, r.image, r.binning):
        if cb.tensor is not None:
            cb.tensor.zero_()
    r.out_color.zero_()
    img = r.draw(cam, count_staged=True, **kw).cpu().numpy().copy()
    return r, img


def compare_inria(r, img, exp, what, lists=True, colors_given=False, rows=None):
    """Everything one upstream-profile call leaves behind against oracle/inria_np.forward's (blend_with="cpp" or "numpy-expf":
    libm's exponential): radii, tilesTouched, pointOffsets, means2D, depths, cov3D, conicOpacity, rgb and the clamp flags bit
    for bit (a Gaussian without a tile: zeros in all of them), num_rendered, the sorted keys / values, the ranges, then
    assert_blend_parity with finalT and nContrib bit for bit, and the staged records.
    lists=False: the call ran with sorted_lists=False and left none (the stamp is checked instead). colors_given: the call took
    colors_precomp, so rgb / clamped are not written (zeros). rows: (y0, y1) pixel rows a tile-row band call wrote."""
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    assert np.array_equal(g["radii"], exp["radii"]), what
    assert np.array_equal(g["tilesTouched"].view(np.uint32), exp["tilesTouched"]), what
    assert np.array_equal(g["pointOffsets"].view(np.uint32), exp["pointOffsets"]), what
    bit_equal = {}
    for k in ("means2D", "depths", "cov3D", "conicOpacity", "rgb"):
        e = np.zeros_like(exp[k]) if (k == "rgb" and colors_given) else exp[k]
        bit_equal[k] = bool(np.array_equal(g[k].view(np.uint32), np.ascontiguousarray(e, np.float32).view(np.uint32)))
    print(f"[inria] {what}: " + ", ".join(f"{k} {'bit-equal' if v else 'DIFFERS'}" for k, v in bit_equal.items()))
    for k, v in bit_equal.items():
        assert v, (what, k, np.nonzero((g[k] != exp[k]).reshape(len(g[k]), -1).any(1))[0][:8])
    assert np.array_equal(g["clamped"], np.zeros_like(exp["clamped"]) if colors_given else exp["clamped"]), what
    no_tile = exp["tilesTouched"] == 0
    for k in ("radii", "means2D", "depths", "cov3D", "conicOpacity", "rgb", "clamped"):
        assert not g[k][no_tile].any(), (what, k, "a Gaussian without a tile keeps zeros")
    R = exp["num_rendered"]
    assert r.last_num_rendered == R == exp["keys"].size, (what, r.last_num_rendered, R)
    if R > 0:
        b = r.map_binning_state()
        if lists:
            assert r.last_lists_written, what
            assert np.array_equal(b["keys"].cpu().numpy().view(np.uint64), exp["keys"]), what
            assert np.array_equal(b["values"].cpu().numpy().view(np.uint32), exp["values"]), what
        else:
            assert not r.last_lists_written and (int(b["values"][0]) & 0xFFFFFFFF) == 0xFFFFFFFF, what
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    assert np.array_equal(im["ranges"].view(np.uint32), exp["ranges"]), what
    ys = slice(None) if rows is None else slice(rows[0], rows[1])
    sub = {k: exp[k][..., ys, :] for k in ("out_color", "finalT", "nContrib")}
    err = assert_blend_parity(img[:, ys], im["finalT"][ys], im["nContrib"][ys], sub, what, bitwise_t=True)
    assert r.last_records_staged == exp["records_staged"], (what, r.last_records_staged, exp["records_staged"])
    return err
