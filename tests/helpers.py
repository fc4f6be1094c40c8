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


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class HostForwardState:
    """The forward state of oracle/cpu_oracle.forward (the state the GPU reproduces bit for bit) behind the part of
    SplatRasterizer's interface that oracle_gradients and block_feed_facts read: scenes are tuned, and their preconditions
    checked, without a GPU."""

    def __init__(self, state, cam):
        self.state, self.width, self.height = state, cam.width, cam.height
        self.num_gaussians = int(state["means2D"].shape[0])
        self.last_num_rendered = int(state["num_rendered"])
        self.out_color = state["out_color"]

    def map_geometry_state(self):
        return {k: self.state[k] for k in ("means2D", "conicOpacity", "rgb", "tilesTouched", "depths", "radii")}

    def map_image_state(self):
        return {k: self.state[k] for k in ("ranges", "nContrib", "finalT")}

    def map_binning_state(self):
        return {"values": self.state["values"]}


def oracle_gradients(r, dL, bg, tiles, targets, max_depth, bad_pixels=None, f32_forward=False, magnitudes=False, t_cutoff=0.001,
                     full_lists=False, colors=None, background=None, group_of_tile=None, threads=1):
    """Float64 gradients (oracle/backward_np.blend_tile_backward) of the Gaussians `targets`, summed over `tiles` (which must
    contain every tile those Gaussians touch), from the forward state of the rasterizer `r` (its means2D, conics, colours and
    sorted lists; or a HostForwardState). Returns a dict:
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
    enough when the GPU's nContrib is right, which the caller must then check on its own).
    colors [N,3] / background: composited instead of the state's rgb and `bg` (the depth channel's pass: colours (d_i, 0, 0)
    over a zero background; the image is then not compared with the state's).
    group_of_tile (needs magnitudes): int[tiles of the frame], a group number per tile (-1: none). The result then also holds
    `groups`: {g: {exp, M, k, pixels, free_pixels, tiles}}, the same sums over the tiles of group g alone, and `tile_group`,
    the argument — what restricted_reference() composes the reference of a part of the frame from.
    threads: tiles evaluated side by side on that many host threads (numpy leaves the interpreter lock in its array loops); the
    sums are added in the order of `tiles` whatever it is."""
    from oracle import backward_np as B
    W, H = r.width, r.height
    gx = (W + 15) // 16
    geo = r.map_geometry_state()
    means2D, conic = _np(geo["means2D"]), _np(geo["conicOpacity"])
    rgb = _np(geo["rgb"]) if colors is None else np.asarray(colors)
    bg_used = bg if background is None else background
    image = r.map_image_state()
    ranges = _np(image["ranges"]).view(np.uint32).astype(np.int64)
    ncontrib = _np(image["nContrib"]).view(np.uint32).astype(np.int64)
    plist = _np(r.map_binning_state()["values"]).view(np.uint32).astype(np.int64)
    final_t = _np(image["finalT"])
    out_color = _np(r.out_color) if colors is None and background is None else None
    row_of = np.full(r.num_gaussians, -1, np.int64)
    row_of[targets] = np.arange(len(targets))
    n = len(targets)
    dims = {"dL_dmean2D": 2, "dL_dconic": 3, "dL_dcov2D": 3, "dL_dopacity": 1, "dL_dcolors": 3}

    def empty():
        return {"exp": {k: np.zeros((n, d)) for k, d in dims.items()}, "M": {k: np.zeros((n, d)) for k, d in dims.items()},
                "k": np.zeros(n, np.int64), "pixels": np.zeros(n, np.int64), "free_pixels": np.zeros(n, np.int64),
                "tiles": np.zeros(n, np.int64)}
    total = empty()
    groups = {}
    assert group_of_tile is None or magnitudes
    nc_frame, ft_frame, stop_frame = np.full((H, W), -1, np.int64), np.full((H, W), np.nan), np.full((H, W), -1, np.int64)
    differs_px = []
    dL_host = _np(dL)
    def evaluate(tile):
        tx, ty = tile
        t = ty * gx + tx
        ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
        nc_tile = ncontrib[ya:yb, xa:xb]
        a = int(ranges[t, 0])
        length = max(0, int(ranges[t, 1]) - a)
        depth = length if full_lists else int(nc_tile.max())     # the list prefix that reaches every pixel's last contributor
        assert depth <= length and depth <= max_depth, (depth, length, max_depth)
        ids = plist[a:a + depth]
        tile_g = np.zeros((3, 16, 16))
        tile_g[:, : yb - ya, : xb - xa] = dL_host[:, ya:yb, xa:xb]
        return ids, B.blend_tile_backward(means2D[ids], conic[ids], rgb[ids], tx, ty, W, H, bg_used, tile_g, t_cutoff=t_cutoff,
                                          f32_forward=f32_forward, magnitudes=magnitudes)
    if threads > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(threads) as pool:
            evaluated = list(pool.map(evaluate, tiles))
    else:
        evaluated = map(evaluate, tiles)
    for (tx, ty), (ids, res) in zip(tiles, evaluated):
        t = ty * gx + tx
        ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
        nc_tile = ncontrib[ya:yb, xa:xb]
        differs = res["n_contrib"][: yb - ya, : xb - xa] != nc_tile
        bad = int(differs.sum())
        differs_px.extend((ya + int(y), xa + int(x)) for y, x in zip(*np.nonzero(differs)))
        if bad_pixels is not None:
            ft = final_t[ya:yb, xa:xb].astype(np.float64)
            differs = differs | (np.abs(res["final_t"][: yb - ya, : xb - xa] - ft) > 1e-5 + 1e-3 * ft)
            bad_pixels.extend((ya + int(y), xa + int(x)) for y, x in zip(*np.nonzero(differs)))
        if bad == 0 and out_color is not None:   # float32 chain of up to 10 000 records against float64: sanity only (parity is the C++ oracle's job)
            assert np.abs(res["out"][:, : yb - ya, : xb - xa] - out_color[:, ya:yb, xa:xb]).max() <= 3e-3
        rows = row_of[ids]
        hit = rows >= 0
        into = [total]
        if group_of_tile is not None and group_of_tile[t] >= 0:
            into.append(groups.setdefault(int(group_of_tile[t]), empty()))
        for acc in into:
            for key, d, m in _GRAD_KEYS:
                np.add.at(acc["exp"][key], rows[hit], res[d][hit].reshape(-1, dims[key]))
                if magnitudes:
                    np.add.at(acc["M"][key], rows[hit], res[m][hit].reshape(-1, dims[key]))
            if magnitudes:
                np.maximum.at(acc["k"], rows[hit], res["k"][hit])
                np.add.at(acc["pixels"], rows[hit], res["pixels"][hit])
                np.add.at(acc["free_pixels"], rows[hit], res["free_pixels"][hit])
                np.add.at(acc["tiles"], rows[hit], (res["pixels"][hit] > 0).astype(np.int64))
        if magnitudes:
            nc_frame[ya:yb, xa:xb] = res["n_contrib"][: yb - ya, : xb - xa]
            ft_frame[ya:yb, xa:xb] = res["final_t"][: yb - ya, : xb - xa]
            stop_frame[ya:yb, xa:xb] = res["stop_idx"][: yb - ya, : xb - xa]
    out = {"exp": total["exp"], "differs": differs_px}
    if magnitudes:
        out.update(M=total["M"], k=total["k"], pixels=total["pixels"], free_pixels=total["free_pixels"], tiles=total["tiles"],
                   n_contrib=nc_frame, final_t=ft_frame, stop_idx=stop_frame)
    if group_of_tile is not None:
        out.update(groups=groups, tile_group=np.asarray(group_of_tile), n_targets=n)
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
# The block feed on frames of several blocks (tests/test_gpu_backward_blocks.py, one MI355X; the bound unchanged, no term added —
# the float flush of a per-entry sum is one more float addition per block of the Gaussian, at most six here, inside BW_C):
# worst |err| / ((k + 8 [+ tiles where a block of the Gaussian is per-entry, or wide_sums=False]) M), scene A12: block lists
# 2.34e-8, with float sums 2.16e-8, beside sorted lists 2.34e-8, band through a block 2.34e-8, second call 2.34e-8 (both calls);
# A13: 2.13e-8, 2.04e-8, 2.13e-8, 2.01e-8, 2.13e-8 in that order, upstream profile 2.43e-8; with the depth channel (kAcc = 13; depth
# and inverse depth alike) A12 wide / float sums 2.34e-8 / 2.16e-8, dL_ddepths 2.05e-8 / 2.00e-8; A13 2.13e-8 / 2.05e-8, dL_ddepths
# 1.96e-8 / 1.92e-8; scene C (a block of 65 units, direct atomics) 2.69e-8 wide, 2.56e-8 float.
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
    per-entry sums): the tiles term is added (a bool, or bool[n]: for the Gaussians it holds of). got: gradients_of(...). Returns the worst ratio |got - exp| / ((k + BW_C [+ tiles]) M)
    over the components with M > 0 (printed; where M = 0 the bound is BW_ATOL)."""
    exp, M = ref["exp"], ref["M"]
    none = ref["pixels"] == 0
    clamped = (ref["pixels"] > 0) & (ref["free_pixels"] == 0)
    float_tile_sums = np.asarray(float_tile_sums, bool)
    depth = ref["k"].astype(np.float64) + BW_C + np.where(float_tile_sums, ref["tiles"].astype(np.float64), 0.0)
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
          f"|err| / ((k + c{' + tiles' if float_tile_sums.any() else ''}) M) = {worst:.3e} at {worst_at}")
    return worst


# ---- the block-list feed of the render backward on frames of several blocks (tests/test_gpu_backward_blocks.py) ----
K_TILES_PER_BLOCK = 8          # csrc/blockbin.hpp: kBW = kBH
K_UNIT = 2048                  # kUnit: block-list entries per unit
K_ACC_MAX_UNITS = 2            # csrc/backward.hip: kAccMaxUnits


def pixel_splats(cam, px, py, z, sigma_px, opacity, dc):
    """test_gpu_backward_edges._splats for isotropic splats, vectorised (its per-row solve takes 7 s for 133 000 rows): the
    scene of n splats whose centres project to the pixel positions (px, py) at world depth z for the axis-aligned default
    camera (the map from world (X, Y) to the pixel is affine at a fixed z: three projections and Cramer's rule), sigma_px the
    3-D scale as pixels at that depth. All arguments arrays [n] (dc [n,3])."""
    from oracle import backward_np as B
    px, py, z, sig = (np.asarray(v, np.float64) for v in (px, py, z, sigma_px))
    n = px.size
    zero, one = np.zeros(n), np.ones(n)
    P = lambda X, Y: B.project_mean2d((X, Y, z), cam.proj, cam.width, cam.height)
    o = P(zero, zero)
    ex, ey = P(one, zero) - o, P(zero, one) - o
    bx, by = px - o[0], py - o[1]
    det = ex[0] * ey[1] - ey[0] * ex[1]
    focal = cam.height / (2.0 * cam.tan_fovy)
    means = np.ones((n, 4), np.float32)
    means[:, 0] = (bx * ey[1] - ey[0] * by) / det
    means[:, 1] = (ex[0] * by - bx * ex[1]) / det
    means[:, 2] = z
    scales = np.full((n, 4), np.e, np.float32)
    scales[:, :3] = (np.maximum(sig, 1e-4) * (z + 5.0) / focal)[:, None]       # (camera at z = -5)
    rots = np.zeros((n, 4), np.float32)
    rots[:, 0] = 1.0
    shs = np.zeros((n, 48), np.float32)
    shs[:, :3] = dc
    return {"means3D": means, "scales": scales, "rotations": rots, "opacities": np.asarray(opacity, np.float32), "shs": shs}


def _rows(rng, n, x, y, z, sig, op):
    """n rows (px, py, z, sigma_px, opacity, dc[3]) drawn uniformly from the given (lo, hi) ranges."""
    u = lambda lo_hi: rng.uniform(lo_hi[0], lo_hi[1], n)
    return np.concatenate([np.stack([u(x), u(y), u(z), u(sig), u(op)], 1), rng.uniform(-1, 1, (n, 3))], 1)


def _opaque_stacks(rng, n_stacks, x, y, per_stack=8):
    """Stacks of nearly opaque splats at nearly the same pixel, in front of everything else: the pixels under them end early."""
    rows = []
    for _ in range(n_stacks):
        cx, cy = rng.uniform(*x), rng.uniform(*y)
        r = _rows(rng, per_stack, (cx - 0.4, cx + 0.4), (cy - 0.4, cy + 0.4), (-2.0, -1.5), (1.5, 3.0), (0.8, 0.97))
        rows.append(r)
    return np.concatenate(rows)


BLOCK_SCENE_A_SIZE = (272, 144)      # 17 x 9 tiles: 3 x 2 blocks, the last block column one tile wide, the last block row one high
BLOCK_SCENE_A_FILL = {"A12": 390, "A13": 540}      # n_fill, chosen on the CPU (tests/test_backward_block_scenes_cpu.py)


def block_scene_camera(w, h):
    from gsrast_amd import camera
    return camera.default_camera(w, h, near=0.05, far=50.0)


def block_scene_a(n_fill, seed=31):
    """Scene A of tests/test_gpu_backward_blocks.py (see there): (scene, camera). n_fill: the frame-wide faint splats, each an
    entry of all six blocks with a hundred-odd instances — the knob for R / E_total."""
    w, h = BLOCK_SCENE_A_SIZE
    cam = block_scene_camera(w, h)
    rng = np.random.default_rng(seed)
    parts = [
        # block (0,0), deep: tiny faint splats, more than two units of them, no pixel ends early
        _rows(rng, 4400, (4, 124), (4, 124), (-1.0, 1.0), (0.2, 0.6), (0.01, 0.05)),
        # block (1,0), two units: small faint splats, and opaque stacks in front
        _rows(rng, 2300, (133, 251), (4, 123), (-1.0, 1.0), (0.5, 2.0), (0.01, 0.1)),
        _opaque_stacks(rng, 6, (140, 245), (10, 118)),
        # the edge blocks (2,0), (0,1), (1,1), (2,1): ordinary splats and opaque stacks
        _rows(rng, 220, (258, 271), (2, 126), (-1.0, 1.0), (1.0, 4.0), (0.05, 0.9)),
        _opaque_stacks(rng, 3, (258, 270), (8, 120)),
        _rows(rng, 220, (2, 126), (130, 143), (-1.0, 1.0), (1.0, 4.0), (0.05, 0.9)),
        _opaque_stacks(rng, 3, (8, 120), (130, 142)),
        _rows(rng, 220, (130, 254), (130, 143), (-1.0, 1.0), (1.0, 4.0), (0.05, 0.9)),
        _opaque_stacks(rng, 3, (136, 250), (130, 142)),
        _rows(rng, 60, (257, 271), (129, 143), (-1.0, 1.0), (1.0, 4.0), (0.05, 0.9)),
        _opaque_stacks(rng, 1, (260, 268), (132, 140)),
    ]
    # splats on the block corners and edges: entries of two or four blocks
    for cx, cy in ((128, 128), (256, 128), (128, 64), (64, 128)):
        parts.append(_rows(rng, 3, (cx - 2, cx + 2), (cy - 2, cy + 2), (-1.0, 1.0), (6.0, 12.0), (0.1, 0.6)))
    # frame-wide faint splats, a third of them behind everything else: centred so that 3 sigma reaches all six blocks
    sig = rng.uniform(25.0, 60.0, n_fill)
    reach = 3.0 * sig
    fill = np.concatenate([np.stack([192.0 + rng.uniform(-0.8, 0.8, n_fill) * (reach - 70.0),
                                     np.maximum(136.0 - reach, 8.0) + rng.uniform(0.0, 1.0, n_fill) * (128.0 - np.maximum(136.0 - reach, 8.0)),
                                     np.where(rng.uniform(size=n_fill) < 1.0 / 3.0, rng.uniform(1.2, 1.5, n_fill), rng.uniform(-1.0, 1.0, n_fill)),
                                     sig, rng.uniform(0.006, 0.02, n_fill)], 1), rng.uniform(-1, 1, (n_fill, 3))], 1)
    parts.append(fill)
    rows = np.concatenate(parts)
    return pixel_splats(cam, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:8]), cam


BLOCK_SCENE_C_TILES = ((0, 0), (7, 0), (0, 7), (7, 7), (3, 4), (5, 2))      # the block's corner tiles and two interior ones


def block_scene_c(n=133000, n_outside=200, seed=32):
    """Scene C: one block of 128 x 128 pixels whose list has more than 64 units (64 x 2048 = 131 072 entries): tiny faint splats
    at random depths, and a few that project outside the frame (no tile: their gradients stay zero bit for bit)."""
    w = h = 128
    cam = block_scene_camera(w, h)
    rng = np.random.default_rng(seed)
    rows = np.concatenate([_rows(rng, n, (0, w), (0, h), (-1.0, 1.0), (0.2, 0.2), (0.01, 0.02)),
                           _rows(rng, n_outside, (-60, -40), (0, h), (-1.0, 1.0), (0.2, 0.2), (0.01, 0.02))])
    return pixel_splats(cam, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:8]), cam


def block_scene_gradient(w, h, seed=17):
    """(dL_dout [3,h,w], dL_ddepth [h,w]) float32: the image gradients every test of the block scenes uses."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3, h, w)).astype(np.float32), rng.normal(size=(h, w)).astype(np.float32)


def block_feed_facts(r, rows=None, depth=False):
    """Which way every block of a block-fed frame takes to the per-Gaussian sums in gsr_backward (csrc/backward.hip,
    block_acc_fits), derived on the host from the forward state of `r` (a SplatRasterizer after draw(plan="sort") of the whole
    frame, or a HostForwardState): its sorted lists, nContrib and depths.
    The entries of block b are the Gaussians whose tile rectangle (clipped to the rows of a band call) meets the block
    (csrc/blockbin.hip, coarse_count_kernel: one entry per block the rectangle meets) — the sorted lists hold one record per
    tile of the rectangle, so: the distinct Gaussians in the lists of the block's tiles — in (depth bits, index) order, the
    order of the depth sort they are filtered from. list_start()[nbp] is their total E_total. p_b: the position in block b's
    list of the deepest last contributor of its tiles; BlockMeta::walked[b], the units the block-fed forward blend looked into,
    lies between ceil((p_b + 1) / 2048) and ceil(E_b / 2048). So with kAcc = 12 (13 with the depth channel) and the 2 R floats
    of scratch the way is
      "per_entry"  for certain if kAcc E_total <= 2 R and E_b <= 2 x 2048,
      "direct"     for certain if kAcc E_total > 2 R or p_b >= 2 x 2048,
      None         otherwise (it depends on how far the blend looked: a test must not rest on such a block).
    rows: (row_begin, row_end), the tile rows of a band call: R and the entries are the band's own (a band call bins only its
    rows; the lists of its tiles are those of the full frame).
    Returns dict: R, E_total, k_acc, fits, blocks {(bx, by): {E, p, way, entries (indices in list order), tiles}},
    membership {gaussian index: [(bx, by), ...]}, nbx, nby."""
    W, H = r.width, r.height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nbx, nby = (gx + K_TILES_PER_BLOCK - 1) // K_TILES_PER_BLOCK, (gy + K_TILES_PER_BLOCK - 1) // K_TILES_PER_BLOCK
    image = r.map_image_state()
    ranges = _np(image["ranges"]).view(np.uint32).astype(np.int64)
    ncontrib = _np(image["nContrib"]).view(np.uint32).astype(np.int64)
    plist = _np(r.map_binning_state()["values"]).view(np.uint32).astype(np.int64)
    depth_bits = _np(r.map_geometry_state()["depths"]).astype(np.float32).view(np.uint32).astype(np.int64)
    row0, row1 = (0, gy) if rows is None else rows
    k_acc = 13 if depth else 12
    blocks, R = {}, 0
    for by in range(nby):
        for bx in range(nbx):
            tiles = [(tx, ty) for ty in range(max(row0, by * K_TILES_PER_BLOCK), min(row1, gy, (by + 1) * K_TILES_PER_BLOCK))
                     for tx in range(bx * K_TILES_PER_BLOCK, min(gx, (bx + 1) * K_TILES_PER_BLOCK))]
            lists = {t: plist[ranges[t[1] * gx + t[0], 0]:ranges[t[1] * gx + t[0], 1]] for t in tiles}
            R += sum(len(v) for v in lists.values())
            ids = np.unique(np.concatenate(list(lists.values()))) if lists else np.zeros(0, np.int64)
            entries = ids[np.lexsort((ids, depth_bits[ids]))]
            pos = {int(g): i for i, g in enumerate(entries)}
            p = -1
            for (tx, ty), lst in lists.items():
                m = int(ncontrib[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].max())
                assert m <= len(lst)
                # (the tile's list is a filter of the block's list in the same order: checked, the derivation rests on it)
                assert (np.diff([pos[int(g)] for g in lst]) > 0).all(), ("a tile list out of block-list order", bx, by, tx, ty)
                if m > 0:
                    p = max(p, pos[int(lst[m - 1])])
            blocks[(bx, by)] = {"E": len(entries), "p": p, "entries": entries, "tiles": tiles}
    E_total = sum(b["E"] for b in blocks.values())
    fits = k_acc * E_total <= 2 * R
    membership = {}
    for key, b in blocks.items():
        b["way"] = ("per_entry" if fits and b["E"] <= K_ACC_MAX_UNITS * K_UNIT else
                    ("direct" if (not fits) or b["p"] >= K_ACC_MAX_UNITS * K_UNIT else None))
        for g in b["entries"]:
            membership.setdefault(int(g), []).append(key)
    return {"R": R, "E_total": E_total, "k_acc": k_acc, "fits": fits, "blocks": blocks, "membership": membership, "nbx": nbx, "nby": nby}


def describe_block_ways(facts):
    return (f"R {facts['R']}, E_total {facts['E_total']}, R / E_total {facts['R'] / max(1, facts['E_total']):.3f}, kAcc {facts['k_acc']}; " +
            ", ".join(f"{k}: E {b['E']} p {b['p']} {b['way']}" for k, b in facts["blocks"].items()))


def assert_block_ways(facts, expected, what=""):
    """Every block's way is certain, and is what the scene is meant to hit. expected: {(bx, by): way}, or one way for all."""
    msg = f"{what}: {describe_block_ways(facts)}"
    for key, b in facts["blocks"].items():
        assert b["way"] is not None, ("a block whose way depends on how far the forward blend looked: retune the scene", key, msg)
        want = expected if isinstance(expected, str) else expected.get(key)
        assert want is None or b["way"] == want, (key, want, msg)


def float_sum_gaussians(facts, targets):
    """bool[len(targets)]: Gaussians with an entry in a per-entry block (their sums pass through float sums over the block's tiles)."""
    per_entry = {k for k, b in facts["blocks"].items() if b["way"] == "per_entry"}
    return np.array([any(k in per_entry for k in facts["membership"].get(int(g), ())) for g in targets], bool)


def block_group_of_tile(w, h, split_row=None):
    """int[tiles]: group = 2 x block number + (1 if the tile's row >= split_row else 0): the tiles of one block inside and outside
    a band that starts at tile row split_row (block number = by nbx + bx)."""
    gx, gy = (w + 15) // 16, (h + 15) // 16
    nbx = (gx + K_TILES_PER_BLOCK - 1) // K_TILES_PER_BLOCK
    out = np.zeros(gx * gy, np.int64)
    for ty in range(gy):
        for tx in range(gx):
            b = (ty // K_TILES_PER_BLOCK) * nbx + tx // K_TILES_PER_BLOCK
            out[ty * gx + tx] = 2 * b + (1 if split_row is not None and ty >= split_row else 0)
    return out


def restricted_reference(ref, keep, w, h):
    """The reference of oracle_gradients(..., group_of_tile=...) over the tiles of the groups `keep` alone, in oracle_gradients'
    own layout (n_contrib / final_t / stop_idx: -1 / NaN / -1 outside those tiles)."""
    n = ref["n_targets"]
    dims = {key: ref["exp"][key].shape[1] for key, _, _ in _GRAD_KEYS}
    out = {"exp": {k: np.zeros((n, d)) for k, d in dims.items()}, "M": {k: np.zeros((n, d)) for k, d in dims.items()},
           "k": np.zeros(n, np.int64), "pixels": np.zeros(n, np.int64), "free_pixels": np.zeros(n, np.int64), "tiles": np.zeros(n, np.int64)}
    for g in keep:
        part = ref["groups"].get(int(g))
        if part is None:
            continue
        for key in dims:
            out["exp"][key] += part["exp"][key]
            out["M"][key] += part["M"][key]
        out["k"] = np.maximum(out["k"], part["k"])
        for key in ("pixels", "free_pixels", "tiles"):
            out[key] = out[key] + part[key]
    gx = (w + 15) // 16
    on = np.isin(ref["tile_group"], list(keep)).reshape(-1, gx)
    mask = np.repeat(np.repeat(on, 16, 0), 16, 1)[:h, :w]
    out["n_contrib"] = np.where(mask, ref["n_contrib"], -1)
    out["final_t"] = np.where(mask, ref["final_t"], np.nan)
    out["stop_idx"] = np.where(mask, ref["stop_idx"], -1)
    out["differs"] = [(y, x) for y, x in ref["differs"] if mask[y, x]]
    return out


def depth_superposition(ref_c, ref_d):
    """The reference of a backward with the depth channel from two passes of the oracle over the same lists — ref_c: the colour
    pass; ref_d: colours (d_i, 0, 0) against the gradient (dL_ddepth, 0, 0) over a zero background. The blend is linear in
    the colours, and so is every condition scale (sums of absolute values: |col| . |g| + |d_i| |g_d|): expected sums and M are the
    two passes' added — but dL_dcolors, which the depth does not reach — and dL_ddepths is the second pass's dL_dcolors[:, 0]
    with its M (keys "dL_ddepths" of exp and M). Walk depth, pixels and tiles are the lists' own, the same in both."""
    assert np.array_equal(ref_c["k"], ref_d["k"]) and np.array_equal(ref_c["pixels"], ref_d["pixels"])
    assert np.array_equal(ref_c["n_contrib"], ref_d["n_contrib"])
    out = dict(ref_c)
    out["exp"] = {k: ref_c["exp"][k] + (ref_d["exp"][k] if k != "dL_dcolors" else 0.0) for k in ref_c["exp"]}
    out["M"] = {k: ref_c["M"][k] + (ref_d["M"][k] if k != "dL_dcolors" else 0.0) for k in ref_c["M"]}
    out["exp"]["dL_ddepths"] = ref_d["exp"]["dL_dcolors"][:, 0:1].copy()
    out["M"]["dL_ddepths"] = ref_d["M"]["dL_dcolors"][:, 0:1].copy()
    return out


def assert_depth_sums_per_gaussian(got_ddepths, ref, float_tile_sums=False, what=""):
    """dL_ddepths of the Gaussians of `ref` (depth_superposition) under assert_backward_per_gaussian's bound, with the
    depth pass's own condition scale; exactly zero where no pixel composites the Gaussian. Returns the worst ratio."""
    e, m = ref["exp"]["dL_ddepths"][:, 0], ref["M"]["dL_ddepths"][:, 0]
    g = np.asarray(got_ddepths, np.float64).reshape(e.shape)
    none = ref["pixels"] == 0
    assert np.isfinite(g).all() and (g[none] == 0.0).all(), (what, "dL_ddepths of a Gaussian no pixel composites")
    depth = ref["k"].astype(np.float64) + BW_C + np.where(np.asarray(float_tile_sums, bool), ref["tiles"].astype(np.float64), 0.0)
    err = np.abs(g - e)
    ratio = np.where(m > 0, err / np.maximum(depth * m, 1e-300), 0.0)
    i = int(np.argmax(ratio))
    over = err > BW_TAU * depth * m + BW_ATOL
    print(f"[backward per Gaussian] {what}, dL_ddepths: worst |err| / ((k + c + tiles) M) = {float(ratio[i]):.3e} at {(i, int(ref['k'][i]), float(e[i]), float(g[i]), float(m[i]))}")
    assert not over.any(), (what, "dL_ddepths", f"{int(over.sum())} Gaussians over the bound; worst ratio {float(ratio[i]):.3e}")
    assert np.abs(e).max() > 0
    return float(ratio[i])


def host_snapshot(r):
    """The forward state of the rasterizer's last draw() as a HostForwardState (numpy copies): what the oracle and
    block_feed_facts read, kept while later draws overwrite the chunks."""
    st = {k: _np(v).copy() for k, v in r.map_geometry_state().items() if k in ("means2D", "conicOpacity", "rgb", "tilesTouched", "depths", "radii")}
    st.update({k: _np(v).copy() for k, v in r.map_image_state().items()})
    st["values"] = _np(r.map_binning_state()["values"]).copy()
    st["num_rendered"] = r.last_num_rendered
    st["out_color"] = _np(r.out_color).copy()
    return HostForwardState(st, r)


def backward_bound(ref, float_tile_sums=True):
    """{key: [n, d]} the bound of assert_backward_per_gaussian (with the tiles term: the widest it applies)."""
    depth = ref["k"].astype(np.float64) + BW_C + (ref["tiles"].astype(np.float64) if float_tile_sums else 0.0)
    return {key: BW_TAU * depth[:, None] * ref["M"][key] + BW_ATOL for key, _, _ in _GRAD_KEYS}


def bound_left_by(ref, faulted_exp, factor=10.0):
    """bool[n]: the Gaussians on which the faulted reference `faulted_exp` (keyed like ref["exp"]) differs from the true one by
    more than `factor` times assert_backward_per_gaussian's bound in some component: where that check would see the fault
    (blindness guards, in the style of chain_seen)."""
    bound = backward_bound(ref)
    seen = np.zeros(len(ref["k"]), bool)
    for key, _, _ in _GRAD_KEYS:
        seen |= (np.abs(faulted_exp[key] - ref["exp"][key]) > factor * bound[key]).any(1)
    return seen


def without_groups(ref, rows, drop):
    """ref["exp"] with, for the Gaussians `rows` (bool [n] or indices), the shares of the groups `drop` taken out."""
    out = {k: v.copy() for k, v in ref["exp"].items()}
    for g in drop:
        part = ref["groups"].get(int(g))
        if part is not None:
            for k in out:
                out[k][rows] -= part["exp"][k][rows]
    return out


def block_blindness_guards_a(ref, facts, targets):
    """The guards of scene A on a reference over the whole frame (oracle_gradients(..., group_of_tile=block_group_of_tile(w, h, 3)),
    targets: every Gaussian): how many Gaussians leave the bound by a factor of 10 when the reference is recomputed
      (a) without the share of one of its blocks (of those where some pixel composites it the one whose share is smallest in
          colour-gradient scale: the hardest to see), for every Gaussian that is an entry of two or more blocks:
          (seen, multi-block Gaussians some pixel composites)
      (b) without the tiles of block column 2 and block row 1
      (c) without the records at block-list positions of 2048 and up in block (1,0).
    Returns {"a": (seen, of), "b": seen, "c": seen}."""
    nbx = facts["nbx"]
    number = lambda key: key[1] * nbx + key[0]
    row_of = {int(g): i for i, g in enumerate(targets)}
    n = len(targets)
    # (a) per Gaussian: drop the block with the smallest (non-zero) share
    dropped = {k: v.copy() for k, v in ref["exp"].items()}
    multi = np.zeros(n, bool)
    for g, keys in facts["membership"].items():
        if len(keys) < 2 or g not in row_of:
            continue
        i = row_of[g]
        shares = []
        for key in keys:
            parts = [ref["groups"].get(2 * number(key) + s) for s in (0, 1)]
            scale = sum(float(p["M"]["dL_dcolors"][i].sum()) for p in parts if p is not None)
            if scale > 0:
                shares.append((scale, key))
        if not shares:
            continue            # no pixel composites it
        multi[i] = True
        _, key = min(shares)
        for s in (0, 1):
            p = ref["groups"].get(2 * number(key) + s)
            if p is not None:
                for k in dropped:
                    dropped[k][i] -= p["exp"][k][i]
    seen_a = bound_left_by(ref, dropped) & multi
    # (b) the edge blocks
    edge = [2 * number(k) + s for k in facts["blocks"] if k[0] == 2 or k[1] == 1 for s in (0, 1)]
    seen_b = bound_left_by(ref, without_groups(ref, slice(None), edge))
    # (c) block (1,0) from its second unit on
    late = np.array([row_of[int(g)] for g in facts["blocks"][(1, 0)]["entries"][K_UNIT:] if int(g) in row_of], np.int64)
    seen_c = bound_left_by(ref, without_groups(ref, late, [2 * number((1, 0)), 2 * number((1, 0)) + 1]))
    return {"a": (int(seen_a.sum()), int(multi.sum())), "b": int(seen_b.sum()), "c": int(seen_c.sum())}


def block_blindness_guard_c(ref, facts, targets):
    """Scene C: the Gaussians that leave the bound by a factor of 10 when the records at block-list positions of 64 x 2048 and
    up are lost (one block: such a Gaussian loses everything)."""
    row_of = {int(g): i for i, g in enumerate(targets)}
    late = np.array([row_of[int(g)] for g in facts["blocks"][(0, 0)]["entries"][64 * K_UNIT:] if int(g) in row_of], np.int64)
    faulted = {k: v.copy() for k, v in ref["exp"].items()}
    for k in faulted:
        faulted[k][late] = 0.0
    return int(bound_left_by(ref, faulted).sum())


def scene_c_targets(r, tiles):
    """The Gaussians whose every tile lies in `tiles` (from the sorted lists and tilesTouched), sorted."""
    gx = (r.width + 15) // 16
    ranges = _np(r.map_image_state()["ranges"]).view(np.uint32).astype(np.int64)
    plist = _np(r.map_binning_state()["values"]).view(np.uint32).astype(np.int64)
    touched = _np(r.map_geometry_state()["tilesTouched"]).view(np.uint32).astype(np.int64)
    ids = np.concatenate([plist[ranges[ty * gx + tx, 0]:ranges[ty * gx + tx, 1]] for tx, ty in tiles])
    g, count = np.unique(ids, return_counts=True)
    return g[count == touched[g]]


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
