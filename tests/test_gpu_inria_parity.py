"""GPU parity of the upstream profile (GSR_FLAG_SEMANTICS_INRIA): the HIP forward against oracle/inria_np.py, whose blend runs
through the C++ oracle's tile loop (libm's expf, cut-off 1e-4). One comparison for every case, helpers.compare_inria: radii,
tilesTouched, pointOffsets, means2D, depths, cov3D, conicOpacity, rgb and the clamp flags bit for bit, num_rendered, the sorted
keys / values, the ranges, finalT and nContrib bit for bit, the staged records, and the pixels within helpers.PIXEL_TOL (the
colour sums are fused; nothing else has a tolerance). Every case asserts that the library took the path it is about and that
the restatement's frame has the property it is about; a precondition that fails is an error, never a skip.

The restatement is this repository's own (no upstream source in the tree): parity of the profile stays unpinned. What is pinned
of the restatement itself is in tests/test_inria_profile.py."""
import functools
import math

import numpy as np
import pytest

from helpers import (single_gaussian_scene, inria_scene, opaque_stack_scene, stop_census, run_inria, compare_inria,
                     assert_blend_parity)
from test_inria_profile import ladder_scene

pytestmark = pytest.mark.gpu

PLAN = "auto"
BG = (0.1, 0.2, 0.3)


@pytest.fixture(autouse=True, params=["sort", "blocks"])
def binning_plan(request):
    """Every case runs under both binning plans (GSR_FLAG_PLAN_SORT / _BLOCKS), as tests/test_gpu_parity.py does."""
    global PLAN
    PLAN = request.param
    yield
    PLAN = "auto"


def _cam(w, h, position=(0.0, 0.0, -5.0), near=0.05, far=50.0):
    from gsrast_amd import camera
    return camera.default_camera(w, h, near=near, far=far, position=position)


def _expect(scene, cam, bg=BG, **kw):
    from oracle import inria_np
    kw.setdefault("blend_with", "cpp")
    kw.setdefault("threads", 8)
    return inria_np.forward(scene, cam, bg, **kw)


def _check(scene, cam, what, bg=BG, exp=None, exp_kw=None, expect_plan=None, **draw_kw):
    """Draws under the module's plan and compares everything with the restatement. Returns (rasterizer, image, expected)."""
    exp = exp if exp is not None else _expect(scene, cam, bg, **(exp_kw or {}))
    draw_kw.setdefault("plan", PLAN)
    r, img = run_inria(scene, cam, bg, **draw_kw)
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    if exp["num_rendered"] > 0:
        assert r.last_plan == (expect_plan or ("generic" if (gx > 255 or gy > 255) else draw_kw["plan"])), (what, r.last_plan)
    compare_inria(r, img, exp, f"{what} plan={r.last_plan}", lists=draw_kw.get("sorted_lists", True),
                  colors_given=draw_kw.get("colors_precomp", False) is not False)
    return r, img, exp


# ---------------------------------------------------------------- plans and feeds
@pytest.mark.parametrize("w,h,n,seed,deg", [(200, 120, 3000, 7, 3), (128, 128, 1500, 3, 1), (333, 257, 8000, 11, 2), (64, 48, 400, 5, 0)])
def test_small_frames_every_output(w, h, n, seed, deg):
    sc = inria_scene(n, seed)
    _, _, exp = _check(sc, _cam(w, h), f"{w}x{h} N={n} deg={deg}", exp_kw=dict(deg=deg), sh_degree=deg)
    assert exp["num_rendered"] > n // 4 and (deg == 0 or exp["clamped"].any())


def test_grid_wider_than_255_tile_columns_takes_the_generic_plan():
    sc = inria_scene(4000, 5, shrink=0.2)
    sc["means3D"][:, 0] *= 12.0
    cam = _cam(4112, 40)
    r, _, exp = _check(sc, cam, "4112x40 (257 tile columns)")
    assert exp["num_rendered"] > 1000 and r.last_plan == "generic"


@functools.lru_cache(maxsize=None)
def _dense():
    """Big splats close up: 48 and more instances per visible Gaussian, where the block plan feeds the blend from its block lists."""
    sc = inria_scene(1500, 31, shrink=0.3)
    sc["scales"][:, :3] = np.random.default_rng(31).uniform(0.25, 0.6, (1500, 3)).astype(np.float32)
    sc["opacities"] = (sc["opacities"] * 0.15).astype(np.float32)
    cam = _cam(640, 360, position=(0.0, 0.0, -3.0))
    return sc, cam, _expect(sc, cam)


@pytest.mark.parametrize("overlap", [False, True])
def test_dense_frame_block_fed_blend_serial_and_overlapped(overlap):
    sc, cam, exp = _dense()
    visible = int((exp["tilesTouched"] > 0).sum())
    assert exp["num_rendered"] >= 48 * visible > 0, (exp["num_rendered"], visible)
    r, _, _ = _check(sc, cam, f"dense, overlap_emit={overlap}", exp=exp, plan="blocks", overlap_emit=overlap)
    assert r.last_plan == "blocks" and not r.last_blend_from_lists and r.last_emit_overlapped == overlap


def test_without_sorted_lists():
    """GSR_FLAG_NO_SORTED_LISTS: pixels, ranges, finalT, nContrib, R and the staged records unchanged; the block plan then
    leaves the stamp in values[0] instead of the lists (the sort plan has nothing to skip and writes them)."""
    sc, cam, exp = _dense()
    skipped = PLAN == "blocks"
    draw = dict(plan=PLAN, sorted_lists=False)
    r, img = run_inria(sc, cam, BG, **draw)
    assert r.last_plan == PLAN and r.last_lists_written == (not skipped)
    compare_inria(r, img, exp, f"sorted_lists=False plan={r.last_plan}", lists=not skipped)


# ---------------------------------------------------------------- blend variants, cut-off and counts
@functools.lru_cache(maxsize=None)
def _stacks():
    sc = opaque_stack_scene()
    cam = _cam(160, 96)
    exp = _expect(sc, cam)
    return sc, cam, exp, stop_census(exp, cam)


@pytest.mark.parametrize("deep", [False, "all", "all8", "all16"])
def test_opaque_stacks_end_between_the_two_cutoffs_under_every_blend_variant(deep):
    """Pixels that stop at 1e-4 and pixels that the other profile's 1e-3 would have stopped and this one does not, faint splats
    around them whose lists are walked to the end: one, four, eight and sixteen waves per tile, each against the restatement."""
    sc, cam, exp, (stop4, stop3_only) = _stacks()
    assert stop4 > 100 and stop3_only > 100
    walked = (exp["finalT"] > 0.5) & (exp["nContrib"] > 0)
    assert walked.sum() > 100                                   # faint splats: composited, far from any cut-off
    r, _, _ = _check(sc, cam, f"opaque stacks deep_tiles={deep}", exp=exp, tile_history=False, deep_tiles=deep)
    assert r.last_deep_tiles == (deep is not False)


def test_nothing_visible_still_writes_the_background():
    sc = single_gaussian_scene(pos=(0, 0, -50.0), n=3)
    cam = _cam(64, 64)
    r, img, exp = _check(sc, cam, "R == 0", bg=(0.2, 0.3, 0.4))
    assert exp["num_rendered"] == 0 and np.array_equal(img[1], np.full((64, 64), np.float32(0.3)))
    r.out_color.fill_(0.9)
    r.draw(cam, semantics="inria", tile_rows=(1, 3), plan=PLAN)
    out = r.out_color.cpu().numpy()
    assert np.array_equal(out[:, 16:48], img[:, 16:48]) and (out[:, :16] == np.float32(0.9)).all() and (out[:, 48:] == np.float32(0.9)).all()


def test_a_single_instance_is_drawn():
    sc = single_gaussian_scene(pos=(0.5178, -0.5178, 0.0), scale=0.001, n=1)
    _, img, exp = _check(sc, _cam(64, 64), "R == 1", bg=(0.2, 0.3, 0.4), exp_kw=dict(deg=0), sh_degree=0)
    assert exp["num_rendered"] == 1 and np.abs(img[0] - 0.2).max() > 1e-3


# ---------------------------------------------------------------- focal lengths
@pytest.mark.parametrize("kx", [1.7, 0.55])
def test_non_square_pixels_use_both_focal_lengths(kx):
    """tan_fovx = kx tan_fovy W / H with the matching projection: focal_x != focal_y. The restatement with the two swapped
    must differ from the kernel, so the case cannot go blind."""
    from gsrast_amd import camera
    w, h = 240, 136
    fov = math.radians(45.0)
    pos = np.array([0.0, 0.0, -5.0], np.float32)
    view = camera.look_at(pos, pos + np.array([0.0, 0.0, 1.0], np.float32), np.array([0.0, -1.0, 0.0], np.float32))
    aspect = np.float32(w) / np.float32(h) * np.float32(kx)
    proj = (camera.perspective(fov, aspect, 0.05, 50.0) @ view).astype(np.float32)
    view = view.copy()
    view[2, :] *= np.float32(-1.0)
    tan_y = float(np.float32(math.tan(np.float32(fov) * np.float32(0.5))))
    cam = camera.Camera(view=np.ascontiguousarray(view.T).reshape(16).copy(), proj=np.ascontiguousarray(proj.T).reshape(16).copy(),
                        cam_pos=pos.copy(), tan_fovx=float(np.float32(tan_y) * aspect), tan_fovy=tan_y, width=w, height=h)
    fx, fy = w / (2.0 * cam.tan_fovx), h / (2.0 * cam.tan_fovy)
    assert abs(fx / fy - 1.0 / kx) < 1e-3
    sc = inria_scene(3000, 13)
    r, _, exp = _check(sc, cam, f"focal_x / focal_y = {fx / fy:.2f}")
    assert exp["num_rendered"] > 1000
    from oracle import inria_np
    swapped = inria_np.preprocess(sc, cam, 3, focal=(np.float32(fy), np.float32(fx)))
    g = r.map_geometry_state()
    assert not np.array_equal(g["conicOpacity"].cpu().numpy(), swapped["conicOpacity"])
    assert not np.array_equal(g["radii"].cpu().numpy(), swapped["radii"])


# ---------------------------------------------------------------- depth keys
@functools.lru_cache(maxsize=None)
def _depth_case(case):
    """Frames by where their depth keys (view-space z) lie relative to the depth sort's main top byte 0x3F, [0.5, 2)."""
    n = 3000
    if case == "all others":
        sc, cam = inria_scene(n, 7), _cam(200, 120, position=(0.0, 0.0, -8.0))
    else:
        sc, cam = inria_scene(n, 7, shrink=0.1), _cam(200, 120, position=(0.0, 0.0, -1.25))
        z = sc["means3D"][:, 2]
        z[:] = np.clip(z, -0.7, 0.7)                                        # view z = z + 1.25 in [0.55, 1.95]
        if case == "a dozen others":
            z[100:106] = np.float32(-0.9) + np.arange(6, dtype=np.float32) * np.float32(0.02)      # view z 0.35 .. 0.45
            z[200:206] = np.float32(0.75) + np.arange(6, dtype=np.float32) * np.float32(0.5)       # view z 2.0 .. 4.5
            sc["means3D"][100:106, :2] *= 0.2
        elif case == "many others":
            z[::2] = np.random.default_rng(1).uniform(1.0, 3.0, z[::2].size).astype(np.float32)
    exp = _expect(sc, cam)
    keys = exp["depths"][exp["tilesTouched"] > 0].view(np.uint32)
    others = (keys >> 24) != 0x3F
    below, beyond = int((keys[others] < np.float32(0.5).view(np.uint32)).sum()), int((keys[others] >= np.float32(2.0).view(np.uint32)).sum())
    return sc, cam, exp, keys.size, below, beyond


@pytest.mark.parametrize("env", [None, ("1", "1"), ("1", "0"), ("0", "1")])
@pytest.mark.parametrize("case", ["main byte only", "a dozen others", "many others", "all others"])
def test_depth_keys_around_the_sorts_main_byte(case, env, library_env):
    """The depth sort's fast route is built for keys whose top byte is 0x3F; under this profile the key is view-space z, so
    every distribution occurs: none outside it, a dozen on both sides (the side list), more than 1 024 (the four-pass fallback),
    nothing else. Each also with the compaction-free first pass and the 12-byte records switched (GSR_FUSED_DEPTH,
    GSR_DEPTH_RECORDS)."""
    sc, cam, exp, visible, below, beyond = _depth_case(case)
    others = below + beyond
    assert visible > 1000
    if case == "main byte only":
        assert others == 0
    elif case == "a dozen others":
        assert below == 6 and beyond == 6
    elif case == "many others":
        assert 1024 < others < visible
    else:
        assert others == visible
    if env is not None:
        library_env(GSR_FUSED_DEPTH=env[0], GSR_DEPTH_RECORDS=env[1])
    _check(sc, cam, f"depth keys: {case} ({below} below 0.5, {beyond} at 2 or beyond, of {visible}), env={env}", exp=exp)


def test_near_plane_to_the_last_bit():
    """Eye at the origin looking down +z: view z is the mean's z exactly. z <= 0.2f is culled: of nextafter(0.2f, 0), 0.2f,
    nextafter(0.2f, 1) and -1 only the third is visible."""
    from gsrast_amd import camera
    cam = camera.first_person_camera((0.0, 0.0, 0.0), 0.0, 0.0, math.radians(45.0), 0.05, 50.0, 96, 64, True)
    sc = single_gaussian_scene(scale=0.01, n=4)
    p2 = np.float32(0.2)
    sc["means3D"][:, 2] = (np.nextafter(p2, np.float32(0)), p2, np.nextafter(p2, np.float32(1)), np.float32(-1.0))
    sc["means3D"][:, 0] = (-0.03, -0.01, 0.01, 0.03)
    _, _, exp = _check(sc, cam, "near plane", exp_kw=dict(deg=0), sh_degree=0)
    assert (exp["tilesTouched"] > 0).tolist() == [False, False, True, False]
    assert exp["depths"][2].view(np.uint32) == sc["means3D"][2, 2].view(np.uint32)


# ---------------------------------------------------------------- the SH sweep through LDS
def _sweep_scene(n, seed):
    """Half of the Gaussians behind the camera: in runs of 128 where n allows (whole waves then skip the sweep), else every
    other one (lanes do); the last one visible, with a negative DC in channel 1 (a clamp) and coefficients in every band."""
    sc = inria_scene(n, seed, sh_scale=0.6, shrink=0.2)
    i = np.arange(n)
    hidden = ((i // 128) % 2 == 1) if n >= 255 else (i % 2 == 1)
    hidden[-1] = False
    sc["means3D"][hidden, 2] = -40.0
    sc["means3D"][-1, :3] = (0.1, -0.1, 0.0)
    sc["shs"][-1, 1] = -6.0
    sc["shs"][-1, 27:48] = np.random.default_rng(seed).uniform(0.5, 1.0, 21).astype(np.float32)    # band 3, every channel
    return sc, hidden


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_sh_sweep_tails_and_degrees(n, deg):
    sc, hidden = _sweep_scene(n, 40 + n)
    cam = _cam(96, 64)
    r, _, exp = _check(sc, cam, f"SH sweep N={n} deg={deg}", exp_kw=dict(deg=deg), sh_degree=deg)
    assert exp["tilesTouched"][-1] > 0 and not (exp["tilesTouched"][hidden] > 0).any()
    assert exp["clamped"][-1, 1] and exp["clamped"].mean() > 0
    if n >= 255:
        assert not (exp["tilesTouched"][128:192] > 0).any()                 # a whole wave without a visible lane
    if deg == 3:
        from oracle import inria_np
        short = sc["shs"].copy()
        short[-1, 44:48] = 0.0                                               # the record's last 16-byte piece
        assert not np.array_equal(inria_np.preprocess(dict(sc, shs=short), cam, 3)["rgb"][-1], exp["rgb"][-1])


@pytest.mark.parametrize("given,same_as", [(-1, 0), (7, 3)])
def test_sh_degree_out_of_range_is_clamped(given, same_as):
    import torch
    sc, _ = _sweep_scene(257, 9)
    cam = _cam(96, 64)
    r, img = run_inria(sc, cam, BG, sh_degree=given, plan=PLAN)
    rgb = r.map_geometry_state()["rgb"].clone()
    img2 = r.draw(cam, semantics="inria", sh_degree=same_as, plan=PLAN, count_staged=True)
    assert torch.equal(rgb.view(torch.int32), r.map_geometry_state()["rgb"].view(torch.int32)) and float(rgb.abs().max()) > 0
    assert np.array_equal(img.view(np.uint32), img2.cpu().numpy().view(np.uint32))
    compare_inria(r, img, _expect(sc, cam, deg=same_as), f"sh_degree {given} -> {same_as}")


# ---------------------------------------------------------------- arguments
@pytest.mark.parametrize("mod", [0.5, 2.0])
def test_scale_modifier(mod):
    sc = inria_scene(3000, 17)
    _, _, exp = _check(sc, _cam(200, 120), f"scale_modifier={mod}", exp_kw=dict(scale_modifier=mod), scale_modifier=mod)
    assert not np.array_equal(exp["radii"], _expect(sc, _cam(200, 120))["radii"])


def test_colours_given_by_the_caller():
    """colors_precomp: composited as given — negative and above one included —, no SH, no clamp flags, cam_pos not needed."""
    import torch
    sc = inria_scene(3000, 19)
    cam = _cam(200, 120)
    cols = np.random.default_rng(19).uniform(-0.5, 1.5, (3000, 3)).astype(np.float32)
    exp = _expect(sc, cam, colors_precomp=cols)
    exp["rgb_used"] = exp["rgb"]
    r, img, _ = _check(sc, cam, "colors_precomp", exp=exp, colors_precomp=torch.from_numpy(cols).to("cuda:0"))
    assert np.abs(img - _expect(sc, cam)["out_color"]).max() > 1e-2


def test_tile_row_bands():
    """Three bands: their union is the whole frame bit for bit, and each band's per-Gaussian state is the restatement's for
    that band — a Gaussian without a tile in the band is invisible (radius 0, zeros), as gsrast_amd.h says."""
    sc = inria_scene(3000, 21)
    sc["means3D"][0, :3] = (0.0, 0.0, -2.0)
    sc["scales"][0, :3] = 3.0                                                # one screen-covering splat
    cam = _cam(640, 360)
    r, full, exp = _check(sc, cam, "bands: whole frame")
    assert exp["tilesTouched"][0] == 40 * 23
    r.out_color.fill_(-1.0)
    for rows in ((0, 7), (7, 8), (8, 23)):
        band = _expect(sc, cam, tile_rows=rows)
        assert 0 < (band["tilesTouched"] > 0).sum() < (exp["tilesTouched"] > 0).sum()
        r.draw(cam, semantics="inria", tile_rows=rows, plan=PLAN, count_staged=True)
        compare_inria(r, r.out_color.cpu().numpy(), band, f"band {rows} plan={r.last_plan}", rows=(16 * rows[0], min(360, 16 * rows[1])))
    assert np.array_equal(r.out_color.cpu().numpy().view(np.uint32), full.view(np.uint32))


# ---------------------------------------------------------------- robustness
@pytest.mark.parametrize("seed", range(6))
def test_extreme_but_finite_inputs(seed):
    """The other profile's test of the same name under this one: scales from 1e-8 to screen-filling and 1e6 : 1 needles,
    quaternions far from unit length (not normalised here: the factor enters the covariance squared, so x 30 and x 1e-3),
    opacities 0, 1, above 1 and below 0, splats on the camera plane, behind the eye and 1e5 units away."""
    from gsrast_amd import camera
    rng = np.random.default_rng(7000 + seed)
    w, h = int(rng.integers(40, 500)), int(rng.integers(40, 300))
    n = int(rng.integers(200, 3000))
    sc = inria_scene(n, 7100 + seed, shrink=0.3)
    pick = lambda frac: rng.random(n) < frac
    s = sc["scales"]
    s[pick(0.05), :3] = 1e-8
    s[pick(0.05), :3] *= 1e3
    needle = pick(0.1)
    s[needle, 0] *= 1e3; s[needle, 1] *= 1e-3
    sc["rotations"][pick(0.1)] *= 30.0
    sc["rotations"][pick(0.1)] *= 1e-3
    op = sc["opacities"]
    op[pick(0.05)] = 0.0; op[pick(0.05)] = 1.0; op[pick(0.03)] = 2.0; op[pick(0.03)] = -0.5; op[pick(0.05)] = 1e-9
    eye = np.array([0.0, 0.0, -1.5]) if seed % 2 else rng.uniform(-1.0, 1.0, 3)
    yaw, pitch = (0.0, 0.0) if seed % 2 else (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.0, 1.0)))
    front = np.array([np.cos(pitch) * np.sin(yaw), np.sin(pitch), np.cos(pitch) * np.cos(yaw)])
    m = sc["means3D"]
    on_plane = pick(0.03)
    m[on_plane, :3] -= (((m[on_plane, :3] - eye) @ front)[:, None] * front[None, :]).astype(np.float32)
    m[pick(0.02), :3] *= 1e5
    cam = camera.first_person_camera(tuple(float(v) for v in eye), yaw, pitch, float(np.radians(45.0)), 0.01, 60.0, w, h, True)
    bg = tuple(float(v) for v in rng.uniform(0, 1, 3))
    exp = _expect(sc, cam, bg)
    assert exp["num_rendered"] > 0, "nothing visible for this seed: choose another"
    for k in ("means2D", "conicOpacity", "cov3D", "depths"):
        assert np.isfinite(exp[k][exp["tilesTouched"] != 0]).all(), f"restatement {k}: not a finite-input case any more"
    _check(sc, cam, f"extreme inputs seed {seed} {w}x{h} N={n}", bg=bg, exp=exp)


def test_non_finite_positions_have_no_tile():
    sc = inria_scene(2000, 23)
    bad = np.arange(5, 2000, 97)
    vals = [np.nan, -np.nan, np.inf, -np.inf]
    for j, i in enumerate(bad):
        sc["means3D"][i, j % 3] = np.float32(vals[j % 4])
    r, img, exp = _check(sc, _cam(200, 120), "NaN / Inf positions")
    assert not (exp["tilesTouched"][bad] > 0).any() and exp["num_rendered"] > 500 and np.isfinite(img).all()


def test_non_finite_and_out_of_range_opacities():
    """NaN, Inf, negative and above-one opacities on visible Gaussians, against the C++ tile loop: its min(0.99, NaN) is 0.99,
    as the reference's and the kernel's. oracle_np.blend is NOT the checker of this case: np.minimum returns NaN there.
    An opacity of -inf is the case that found a fault: far from the centre the exponential underflows to 0, -inf * 0 is NaN
    and the record counts at alpha 0.99, where the blend's footprint filter had dropped every record of opacity <= 0
    (3 093 nContrib and 713 finalT words differed on this frame)."""
    sc = inria_scene(2000, 29)
    exp0 = _expect(sc, _cam(200, 120))
    vis = np.nonzero(exp0["tilesTouched"] > 0)[0]
    assert vis.size > 400
    for j, v in enumerate((np.nan, np.inf, -np.inf, -0.5, 2.0, 1e30)):
        sc["opacities"][vis[j::40]] = np.float32(v)
    _, img, exp = _check(sc, _cam(200, 120), "NaN / out-of-range opacities")
    assert np.isnan(exp["conicOpacity"][vis, 3]).sum() >= 5 and np.isfinite(img).all()


# ---------------------------------------------------------------- mid size
@functools.lru_cache(maxsize=None)
def _mid_size():
    sc = inria_scene(300_000, 53, shrink=0.5)
    cam = _cam(1920, 1080, far=100.0)
    return sc, cam, _expect(sc, cam, threads=16)


def test_mid_size_frame_degree_3():
    sc, cam, exp = _mid_size()
    assert exp["num_rendered"] > 2_000_000
    _check(sc, cam, f"1920x1080 N=300000 R={exp['num_rendered']}", exp=exp)


# ---------------------------------------------------------------- a covariance that overflows: no tile
def test_overflowing_covariances_have_no_tile():
    """Finite scales 1e4 .. 1e19 and quaternion factors 1e3 .. 1e10 among ordinary Gaussians. Where the covariance overflows the
    determinant is Inf or NaN; before the rule such a Gaussian was given every tile of the frame (the radius saturates) or, at
    the far end, radius 0 and one tile, with a conic of zeros or NaNs (profiles/inria_parity.txt has the record, and what the
    blend and the C++ tile loop made of it: not the same). It has no tile, like one behind the camera:
    the frame equals, output for output and pixel for pixel, the frame in which those Gaussians were moved behind the camera;
    no pixel is NaN; gsr_backward returns finite gradients, zeros for them."""
    import torch
    sc, ids = ladder_scene()
    cam = _cam(200, 120)
    r, img, exp = _check(sc, cam, "overflow ladder")
    lost = ids[exp["tilesTouched"][ids] == 0]
    assert 0 < lost.size < ids.size and np.isfinite(img).all()
    moved = {k: v.copy() for k, v in sc.items()}
    moved["means3D"][lost, :3] = (0.0, 0.0, -40.0)
    r2, img2 = run_inria(moved, cam, BG, plan=PLAN)
    g, g2 = r.map_geometry_state(), r2.map_geometry_state()
    for k in g:
        assert torch.equal(g[k].view(torch.uint8), g2[k].view(torch.uint8)), k
    for a, b in ((r.map_binning_state(), r2.map_binning_state()), (r.map_image_state(), r2.map_image_state())):
        for k in ("keys", "values", "ranges", "finalT", "nContrib"):
            if k in a:
                assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert np.array_equal(img.view(np.uint32), img2.view(np.uint32)) and r.last_records_staged == r2.last_records_staged
    dL = torch.from_numpy(np.random.default_rng(2).normal(0, 1, (3, 120, 200)).astype(np.float32)).to("cuda:0")
    grads = r.backward(dL, semantics="inria", sh_degree=3)
    seen = 0
    for k, v in grads.items():
        assert bool(torch.isfinite(v).all()), k
        assert not bool(v[torch.from_numpy(lost).to(v.device)].any()), k
        seen += int(v.abs().sum() > 0)
    assert seen >= 8
