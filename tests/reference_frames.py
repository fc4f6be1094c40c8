"""Frame recipes shared by the tests that compare against the reference compiled for the host (test_reference_pin.py on
the CPU, test_gpu_reference_parity.py on the GPU) and by tests/golden/make_reference_frames.py. Each recipe returns
(scene, camera, background, keyword arguments of the forward call). The recipes of tests/test_gpu_parity.py are restated
here parameter for parameter, so that what the GPU suite checks against the oracle is what the oracle is checked on."""
import numpy as np

from helpers import load_golden, single_gaussian_scene

INT_MIN, INT_MAX = -2147483648, 2147483647

# every output the reference writes (ranges: the tile grid's part of the per-pixel array it allocates)
REF_KEYS = ("radii", "rects", "means2D", "depths", "cov3D", "rgb", "conicOpacity", "tilesTouched", "pointOffsets",
            "keys_unsorted", "values_unsorted", "keys", "values", "ranges", "finalT", "nContrib", "out_color")
PREPROCESS_KEYS = ("radii", "rects", "means2D", "depths", "cov3D", "rgb", "conicOpacity", "tilesTouched")


def golden(use_rects=True):
    scene, cam, bg, _ = load_golden()
    return scene, cam, bg, dict(use_rects=use_rects)


def random_small_frame(seed):
    """test_gpu_parity.test_random_small_frames_against_oracle(seed)."""
    from gsrast_amd import camera, scenes
    rng = np.random.default_rng(1000 + seed)
    w, h = int(rng.integers(17, 700)), int(rng.integers(17, 420))
    if seed % 4 == 0:
        h = int(rng.integers(1, 17))                 # a single tile row
    if seed % 4 == 1:
        w = int(rng.integers(1, 17))                 # a single tile column
    n = int(rng.integers(1, 4000))
    scene = scenes.garden_like_scene(n, seed=2000 + seed)
    scene["means3D"][:, :3] *= float(rng.uniform(0.1, 0.6))
    scene["scales"][:, :3] *= float(np.exp(rng.uniform(-1.0, 2.5)))
    scene["opacities"][:] = rng.uniform(0.01, 1.0, n).astype(np.float32)
    cam = camera.default_camera(w, h, near=0.05, far=50.0)
    bg = tuple(float(v) for v in rng.uniform(0, 1, 3))
    return scene, cam, bg, {}


ANISOTROPIC = [(200, 120, 3000, 7), (333, 257, 20000, 11), (64, 48, 500, 3)]


def anisotropic(w, h, n, seed):
    """test_gpu_parity.test_anisotropic_scenes_against_oracle."""
    from gsrast_amd import camera, scenes
    scene = scenes.garden_like_scene(n, seed=seed)
    scene["means3D"][:, :3] *= 0.25
    return scene, camera.default_camera(w, h, near=0.05, far=50.0), (0.1, 0.2, 0.3), {}


def trained_like_pose(n=6000, w=320, h=192, eye=(0.5, -0.2, -4.0)):
    """The scene family of test_trained_like_scene_against_oracle (flat splats, heavy-tailed scales, bimodal opacity, huge
    background splats), smaller, from inside the cloud."""
    from gsrast_amd import camera, scenes
    scene = scenes.trained_like(n, seed=46)
    return scene, camera.default_camera(w, h, near=0.02, far=120.0, position=eye), (0.1, 0.2, 0.3), {}


def equal_keys():
    from gsrast_amd import camera
    scene = single_gaussian_scene(pos=(0.1, -0.2, 0.3), scale=0.15, opacity=0.3, n=300)
    scene["shs"][:, 0] = np.linspace(-1, 1, 300)
    return scene, camera.default_camera(96, 96), (0.0, 0.0, 0.0), {}


def opaque_stack():
    """1200 records on every tile: past the first 256-entry round; the middle pixels stop early."""
    from gsrast_amd import camera
    n = 1200
    scene = single_gaussian_scene(pos=(0.0, 0.0, 0.0), scale=0.6, opacity=0.95, n=n)
    scene["means3D"][:, 2] = np.linspace(-1.0, 1.0, n)
    return scene, camera.default_camera(64, 64), (0.0, 0.0, 0.0), {}


def single_instance():
    """R == 1: identifyTileRanges never closes the only tile."""
    from gsrast_amd import camera
    scene = single_gaussian_scene(pos=(0.5178, -0.5178, 0.0), scale=0.001, n=1)
    return scene, camera.default_camera(64, 64), (0.2, 0.3, 0.4), {}


def nothing_visible():
    """R == 0: every Gaussian behind the camera."""
    from gsrast_amd import camera
    scene = single_gaussian_scene(pos=(0.0, 0.0, -50.0), n=3)
    return scene, camera.default_camera(64, 64), (0.2, 0.3, 0.4), dict(out_init=np.full((3, 64, 64), 0.25, np.float32))


def wide_grid():
    """4112 x 40 -> 257 x 3 tiles (test_grid_wider_than_255_tiles_uses_generic_digit_passes)."""
    from gsrast_amd import camera, scenes
    scene = scenes.garden_like_scene(4000, seed=5)
    scene["means3D"][:, :3] *= 0.2
    scene["means3D"][:, 0] *= 12.0
    return scene, camera.default_camera(4112, 40, near=0.05, far=50.0), (0.0, 0.1, 0.2), {}


def wide_grid_all_columns():
    """The same 257 x 3 grid with the scene spread over its whole width (wide_grid's recipe reaches 52 of the 257 tile
    columns, none past the 160th): splats in the columns past the 255th."""
    from gsrast_amd import camera, scenes
    scene = scenes.garden_like_scene(4000, seed=5)
    scene["means3D"][:, :3] *= 0.2
    scene["means3D"][:, 0] *= 70.0
    return scene, camera.default_camera(4112, 40, near=0.05, far=50.0), (0.0, 0.1, 0.2), {}


def dense():
    """Big faint splats close up: 48 and more instances per visible Gaussian, where the block plan feeds the blend from its
    block lists instead of the sorted ones."""
    from gsrast_amd import camera, scenes
    scene = scenes.garden_like_scene(1200, seed=31)
    scene["means3D"][:, :3] *= 0.3
    scene["scales"][:, :3] = np.random.default_rng(31).uniform(0.25, 0.6, (1200, 3)).astype(np.float32)
    scene["opacities"] = (scene["opacities"] * 0.15).astype(np.float32)
    return scene, camera.default_camera(480, 272, near=0.05, far=50.0, position=(0.0, 0.0, -3.0)), (0.1, 0.2, 0.3), {}


DEPTH_KEY_CASES = [(0.5, 12), (0.5, 1), (1.3, 0), (3.0, 0), (0.01, 0)]


def depth_keys(near, extra):
    """test_gpu_parity.test_depth_keys_outside_the_main_top_byte."""
    from gsrast_amd import camera, scenes
    n, w, h = 3000, 320, 200
    scene = scenes.garden_like_scene(n, seed=8100)
    scene["means3D"][:, :3] *= 0.25
    scene["scales"][:, :3] *= 2.0
    if extra:
        rng = np.random.default_rng(8101)
        sel = rng.choice(n, extra, replace=False)
        d = rng.uniform(near * 2.2, near * 3.6, extra)
        scene["means3D"][sel, 0] = rng.uniform(-0.05, 0.05, extra) * d
        scene["means3D"][sel, 1] = rng.uniform(-0.05, 0.05, extra) * d
        scene["means3D"][sel, 2] = -5.0 + d
        scene["scales"][sel, :3] = 0.01
    return scene, camera.default_camera(w, h, near=near, far=100.0), (0.0, 0.0, 0.0), {}


def scale_modified(modifier):
    scene, cam, bg, kw = anisotropic(200, 120, 3000, 7)
    return scene, cam, bg, dict(kw, scale_modifier=modifier)


def far_from_unit_quaternions():
    """Every rotation scaled by 1e-3 .. 1e3 (the preprocess re-normalises) and a few by 1e15 / 1e-15."""
    scene, cam, bg, kw = anisotropic(200, 120, 3000, 7)
    rng = np.random.default_rng(31)
    scene["rotations"] *= np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (3000, 1))).astype(np.float32)
    scene["rotations"][::97] *= np.float32(1e15)
    scene["rotations"][5::97] *= np.float32(1e-15)
    return scene, cam, bg, kw


def odd_opacities():
    """Opacities 0, 1, above 1, below 0 and 1e-9 over a quarter of the scene."""
    scene, cam, bg, kw = anisotropic(200, 120, 3000, 7)
    rng = np.random.default_rng(32)
    op = scene["opacities"]
    pick = lambda frac: rng.random(3000) < frac
    op[pick(0.06)] = 0.0; op[pick(0.06)] = 1.0; op[pick(0.05)] = 2.0; op[pick(0.05)] = -0.5; op[pick(0.05)] = 1e-9
    return scene, cam, bg, kw


def on_camera_plane():
    """A tenth of the splats moved onto the camera plane (forward distance exactly 0, or as near as float32 goes): clip
    w = 0, so 1 / (w + 0.001) = 1000 — with the eye inside the cloud."""
    from gsrast_amd import camera, scenes
    n, w, h = 2000, 240, 160
    rng = np.random.default_rng(33)
    scene = scenes.garden_like_scene(n, seed=34)
    scene["means3D"][:, :3] *= 0.3
    eye, yaw, pitch = np.array([0.1, -0.05, -0.4]), 0.3, -0.2
    front = np.array([np.cos(pitch) * np.sin(yaw), np.sin(pitch), np.cos(pitch) * np.cos(yaw)])
    m = scene["means3D"]
    sel = rng.random(n) < 0.1
    m[sel, :3] -= (((m[sel, :3] - eye) @ front)[:, None] * front[None, :]).astype(np.float32)
    cam = camera.first_person_camera(tuple(float(v) for v in eye), yaw, pitch, float(np.radians(45.0)), 0.01, 60.0, w, h, True)
    return scene, cam, (0.3, 0.2, 0.1), {}


def precomputed_inputs(colors=True, cov3d=True, w=64, h=48, n=500):
    """colorsPrecomp and / or cov3DPrecomp given (GSCuda.cu:315-318, :362, :803): covariances of another scene's splats, so
    that they are not what the scales and rotations would give."""
    scene, cam, bg, kw = anisotropic(w, h, n, 3)
    rng = np.random.default_rng(35)
    if colors:
        kw["colors_precomp"] = rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32)
    if cov3d:
        a = rng.normal(0.0, 0.08, (n, 3, 3))
        s = a @ a.transpose(0, 2, 1)
        kw["cov3d_precomp"] = np.stack([s[:, 0, 0], s[:, 0, 1], s[:, 0, 2], s[:, 1, 1], s[:, 1, 2], s[:, 2, 2]], 1).astype(np.float32)
    return scene, cam, bg, kw


# The in-range family bounds the recipe's two scale factors. The largest conversion of a frame is (int) ceil(3.0f * cov.z)
# (GSCuda.cu:352: a variance in pixels squared, no square root), inside int while sigma_y stays below 26 000 pixels. The
# recipe's scales reach 0.8 units, its focal lengths 360 pixels, and a splat is kept down to clip distances of a few
# hundredths: times 1e3 (the unbounded recipe) that is far outside. EXTREME_BOUNDED keeps the needles' 1e6 : 1 and lets the big
# splats cover the screen thousands of times over (extents up to 1.1e9 pixels, half of int's range, against frames of 500); that every conversion
# stayed inside int is asserted per frame from the reference's outputs (conversions_in_range), not assumed from these numbers.
EXTREME_UNBOUNDED = dict(fill=1e3, needle_long=1e3, needle_short=1e-3)
EXTREME_BOUNDED = dict(fill=60.0, needle_long=60.0, needle_short=60e-6)


def extreme_but_finite(seed, fill=1e3, needle_long=1e3, needle_short=1e-3):
    """test_gpu_parity.test_extreme_but_finite_inputs_against_oracle(seed), the factors of the screen-filling splats and of
    the needles as parameters (defaults: that test's)."""
    from gsrast_amd import camera, scenes
    rng = np.random.default_rng(7000 + seed)
    w, h = int(rng.integers(40, 500)), int(rng.integers(40, 300))
    n = int(rng.integers(200, 3000))
    scene = scenes.garden_like_scene(n, seed=7100 + seed)
    scene["means3D"][:, :3] *= 0.3
    pick = lambda frac: rng.random(n) < frac
    sc = scene["scales"]
    sc[pick(0.05), :3] = 1e-8
    sc[pick(0.05), :3] *= fill
    needle = pick(0.1)
    sc[needle, 0] *= needle_long; sc[needle, 1] *= needle_short
    scene["rotations"][pick(0.1)] *= 1e3
    scene["rotations"][pick(0.1)] *= 1e-3
    op = scene["opacities"]
    op[pick(0.05)] = 0.0; op[pick(0.05)] = 1.0; op[pick(0.03)] = 2.0; op[pick(0.03)] = -0.5; op[pick(0.05)] = 1e-9
    eye = np.array([0.0, 0.0, -1.5]) if seed % 2 else rng.uniform(-1.0, 1.0, 3)
    yaw, pitch = (0.0, 0.0) if seed % 2 else (float(rng.uniform(-3.1, 3.1)), float(rng.uniform(-1.0, 1.0)))
    front = np.array([np.cos(pitch) * np.sin(yaw), np.sin(pitch), np.cos(pitch) * np.cos(yaw)])
    m = scene["means3D"]
    on_plane = pick(0.03)
    m[on_plane, :3] -= (((m[on_plane, :3] - eye) @ front)[:, None] * front[None, :]).astype(np.float32)
    m[pick(0.02), :3] *= 1e5
    cam = camera.first_person_camera(tuple(float(v) for v in eye), yaw, pitch, float(np.radians(45.0)), 0.01, 60.0, w, h, True)
    bg = tuple(float(v) for v in rng.uniform(0, 1, 3))
    return scene, cam, bg, {}


def conversions_in_range(out, cam):
    """Whether every float -> int conversion of the frame (GSCuda.cu:240-257, :341 / :370, :352) stayed inside int, from
    the reference's own outputs `out`. The converted extents are the rects and radii themselves: a source outside int (or
    NaN) does not convert to a value strictly inside (INT_MIN, INT_MAX) on any host — x86 gives INT_MIN, a saturating
    host INT_MIN / INT_MAX / 0-for-NaN only where the source was NaN — and the tile-rectangle conversions take
    (mean +- extent + 15) / 16, which an extent inside int and a finite mean keep below 2^28 + |mean| / 16.
    Returns a bool per Gaussian."""
    ok = np.ones(out["radii"].shape[0], bool)
    ext = [out["radii"][:, None]] + ([out["rects"]] if out.get("rects") is not None else [])
    for e in ext:
        e = e.astype(np.int64)
        ok &= ((e > INT_MIN) & (e < INT_MAX)).all(1)
    m = out["means2D"].astype(np.float64)
    ok &= np.isfinite(m).all(1) & (np.abs(m).max(1) < 2.0 ** 30)
    return ok
