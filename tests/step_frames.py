"""The frames of the training-step tests (tests/test_step_autograd_cpu.py, tests/test_gpu_step_autograd.py): the cases, the
scene in raw parameters, the camera, the loss weights, and the reference step of a case (tests/step_autograd_ref.py). And,
in a second table (FULL_CASES, full_*), the frames of tests/test_step_full_cpu.py and tests/test_gpu_step_full.py: the same
pose and size with the 3D filter, the opacity compensation, a feature map and the opacity map, on a scene derived from
raw_scene without altering it. And, in a third table (GEOMETRY_CASES, geometry_*), the frames of
tests/test_step_geometry_cpu.py and tests/test_gpu_step_geometry.py: the same pose, size and sizes of splats with the distortion
map (distortion=, distortion_power), the normal map and the normal-consistency term (normals=True), the median map (median=,
median_threshold), every Gaussian flattened along one axis."""
from __future__ import annotations

import functools

import numpy as np

import step_autograd_ref as R
from step_autograd_ref import RAW

W, H, N = 40, 24, 150                      # 3 x 2 tiles, ragged on both edges; two whole waves and a partial one
BG = (0.2, 0.5, 0.9)
P1 = dict(eye=(2.0, -1.2, -4.2), target=(0.0, 0.0, 0.0), roll=0.4)       # tests/test_gpu_backward_poses.py's pose P1

# name -> (profile, sh_degree, depth, scale_modifier, kx, precomp): the cases of tests/test_gpu_step_autograd.py
CASES = {
    "gscuda": ("gscuda", 0, False, 1.0, 1.0, False),
    "gscuda-depth": ("gscuda", 0, True, 1.0, 1.0, False),
    "gscuda-inverse-m2": ("gscuda", 0, "inverse", 2.0, 1.0, False),
    "inria-3-depth": ("inria", 3, True, 1.0, 1.0, False),
    "inria-0-m0.5": ("inria", 0, False, 0.5, 1.0, False),
    "inria-2-inverse-kx": ("inria", 2, "inverse", 1.0, 1.7, False),
    "inria-precomp": ("inria", 0, False, 1.0, 1.0, True),
}
# the seed of scenes.garden_like_scene and of what raw_scene adds to it, per profile. tests/test_step_autograd_cpu.py checks,
# without a GPU, the conditions a seed must meet: no frame drops more than 1 % of its pixels (these drop none)
SEEDS = {"gscuda": 4, "inria": 4}


def camera_of(case):
    from helpers import posed_camera
    return posed_camera(W, H, kx=CASES[case][4], **P1)


@functools.lru_cache(maxsize=None)
def raw_scene(profile, seed=None):
    """Raw values of the frame's scene: scenes.garden_like_scene shrunk as the pose tests shrink it (positions x 0.25, splats
    four times larger so that they cover pixels), quaternions at lengths 0.5 .. 2, plus
      rows 10..16, 80..86   two stacks of seven nearly opaque splats (the first two of each larger, with opacity 0.9999):
                            pixels under them reach the cut-off and the 0.99 clamp
      rows 20..31, 100..111 behind the camera (culled under either profile)
      rows 140..147         large faint ones beyond 1.3 tan(fov): clamped and visible under the upstream profile (the gscuda
                            profile culls them by their NDC position)
    The upstream profile with all sixteen SH triples, coefficient-major."""
    from gsrast_amd import scenes
    from helpers import posed_camera, world_from_view
    seed = SEEDS[profile] if seed is None else seed
    sc = scenes.garden_like_scene(N, seed=seed)
    rng = np.random.default_rng(seed)
    cam = posed_camera(W, H, **P1)
    xyz = sc["means3D"][:, :3].astype(np.float64) * 0.25
    scale = 4.0 * sc["scales"][:, :3].astype(np.float64)
    opacity = np.clip(sc["opacities"].astype(np.float64), 1e-4, 1.0 - 1e-4)
    quat = sc["rotations"].astype(np.float64)
    tx, ty = cam.tan_fovx, cam.tan_fovy
    for rows, centre in ((np.arange(10, 17), (-0.35, 0.2)), (np.arange(80, 87), (0.4, -0.3))):
        z = np.sort(rng.uniform(2.4, 3.0, rows.size))
        t = np.stack([(centre[0] * tx + rng.uniform(-0.02, 0.02, rows.size)) * z,
                      (centre[1] * ty + rng.uniform(-0.02, 0.02, rows.size)) * z, z], 1)
        xyz[rows] = world_from_view(cam, t)
        scale[rows] = rng.uniform(0.12, 0.25, (rows.size, 3))
        opacity[rows] = rng.uniform(0.9, 0.999, rows.size)
        opacity[rows[:2]] = 0.9999
        scale[rows[:2]] = 0.5
    behind = np.concatenate([np.arange(20, 32), np.arange(100, 112)])
    t = np.stack([rng.uniform(-1, 1, behind.size), rng.uniform(-1, 1, behind.size), -rng.uniform(0.5, 3.0, behind.size)], 1)
    xyz[behind] = world_from_view(cam, t)
    wide = np.arange(140, 148)
    z = rng.uniform(2.5, 4.0, wide.size)
    ratio = np.array([(2.6, 0.3), (-2.5, -0.2), (0.2, 1.7), (-0.4, -1.5), (0.5, 1.6), (-0.2, -1.7), (2.5, 1.45), (-2.45, -1.5)])
    t = np.stack([ratio[:, 0] * tx * z, ratio[:, 1] * ty * z, z], 1)
    xyz[wide] = world_from_view(cam, t)
    beyond = np.maximum(np.abs(ratio[:, 0]) - 1.0, np.abs(ratio[:, 1]) - 1.0) * np.where(np.abs(ratio[:, 0]) > 1.3, tx, ty) * z
    scale[wide] = beyond[:, None] * rng.uniform(1.8, 2.2, (wide.size, 3))
    opacity[wide] = rng.uniform(0.08, 0.2, wide.size)
    raw = {"xyz": xyz.astype(np.float32),
           "opacity_logit": np.log(opacity / (1.0 - opacity)).astype(np.float32),
           "log_scale": np.log(scale).astype(np.float32),
           "rotation": (quat * rng.uniform(0.5, 2.0, (N, 1))).astype(np.float32),
           "shs": sc["shs"].astype(np.float32)}
    if profile == "inria":
        raw["shs"] = rng.normal(0, 0.35, (N, 48)).astype(np.float32)
        raw["shs"][wide, :3] += 2.0
        for r in range(40, 46):                               # a channel clamped at zero at every degree
            raw["shs"][r, r % 3] = -2.5
    raw["colors"] = rng.uniform(0.0, 1.0, (N, 3)).astype(np.float32)          # (the colours of the colors_precomp case)
    return raw


# ---- the frames with the filter, the compensation, the feature map and the opacity map (tests/test_step_full_cpu.py,
# tests/test_gpu_step_full.py). name -> the options of the case; `constant`: the camera tensors that are no leaves (the library
# refuses a view matrix that requires a gradient under antialiased=True); colour=False: the colour's weight is all zeros
def _full(profile, deg, depth, mod=1.0, kx=1.0, filt=False, antialiased=False, channels=0, opacity=False, colour=True):
    return dict(profile=profile, sh_degree=deg, depth=depth, scale_modifier=mod, kx=kx, filter=filt, antialiased=antialiased,
                channels=channels, opacity=opacity, colour=colour, constant=("view",) if antialiased else ())


FULL_CASES = {
    "full-inria": _full("inria", 3, True, filt=True, antialiased=True, channels=5, opacity=True),
    "full-gscuda-m2": _full("gscuda", 0, "inverse", mod=2.0, filt=True, antialiased=True, channels=3, opacity=True),
    "filter-features-kx": _full("inria", 2, "inverse", kx=1.7, filt=True, channels=5, opacity=True),
    "antialias-alone": _full("gscuda", 0, True, antialiased=True),
    "filter-alone": _full("inria", 1, True, filt=True),
    "features-alone": _full("gscuda", 0, False, channels=1, colour=False),
}
# The scene's sizes, in world units (a pixel is about 0.15 at the scene's depth). They are chosen so that the Gaussians whose
# gradients are the largest of the frame are the ones on which the filter and the compensation both matter — splats of about a
# pixel with a filter of their own size: a bound is a share of an array's LARGEST entry, and a cut that only moves the gradients
# of small faint splats beside large opaque ones is not seen (tests/test_step_full_cpu.py, the cuts; raw_scene's own sizes show
# the cut of the smoothed scales inside c by one bound, these by more than a hundred).
FILTER_SCALE = 1.7            # what the training cameras' filter is scaled by: about 0.1, two thirds of a pixel
LARGE_BAND = (0.35, 0.5)      # every other ordinary splat: two to three pixels, hardly compensated ...
LARGE_OPACITY = 0.05          # ... and its opacity multiplied by this, so that it does not set the largest entries
SMALL_BAND = (0.05, 0.12)     # the others: below a pixel, c and the filter's coefficient well below 0.9
STACK_TOP, STACK_SHRINK = 0.08, 0.4     # the two stacks: their first two splats' scale, and the factor on the other five
WIDE_OPACITY = 0.04           # the factor on the opacity of the wide ones (scales of 2 to 8)
IDENTITY_FROM = 7             # rows 7, 17, ... have filter value 0: only two of them lie behind the camera


def full_camera_of(case):
    from helpers import posed_camera
    return posed_camera(W, H, kx=FULL_CASES[case]["kx"], **P1)


def full_scene(case):
    """The scene of a FULL_CASES frame (read-only by convention: it is cached)."""
    return _sized_scene(FULL_CASES[case]["profile"], FULL_CASES[case]["scale_modifier"])


@functools.lru_cache(maxsize=None)
def _sized_scene(profile, scale_modifier):
    """raw_scene(profile), copied, with its ordinary splats (not the stacks, the ones behind the camera or the wide ones)
    brought to the frame's resolution: every other one doubled and clipped into LARGE_BAND, the others clipped into SMALL_BAND
    — but every seventh of those left as it is, far below a pixel. The stacks shrunk to a pixel's size (STACK_TOP,
    STACK_SHRINK), the large and the wide ones fainter (LARGE_OPACITY, WIDE_OPACITY). Under a scale_modifier k every scale is divided by k: the rasterizer sees the same sizes again, and the
    filter, which the modifier multiplies too, is made for them (filter_values). Plus "features" [N,5], standard normal (a
    case of C channels reads the first C columns)."""
    raw = {k: v.copy() for k, v in raw_scene(profile).items()}
    special = np.zeros(N, bool)
    for a, b in ((10, 17), (80, 87), (20, 32), (100, 112), (140, 148)):
        special[a:b] = True
    rows = np.nonzero(~special)[0]
    large, small = rows[::2], np.setdiff1d(rows[1::2], rows[1::2][::7])
    ln = lambda v: np.float32(np.log(v))
    raw["log_scale"][large] = np.clip(raw["log_scale"][large] + ln(2.0), ln(LARGE_BAND[0]), ln(LARGE_BAND[1]))
    raw["log_scale"][small] = np.clip(raw["log_scale"][small], ln(SMALL_BAND[0]), ln(SMALL_BAND[1]))
    raw["log_scale"][[10, 11, 80, 81]] = ln(STACK_TOP)
    for a in (12, 82):
        raw["log_scale"][a:a + 5] += ln(STACK_SHRINK)
    raw["log_scale"] -= ln(scale_modifier)
    for rows_, factor in ((np.arange(140, 148), WIDE_OPACITY), (large, LARGE_OPACITY)):
        o = 1.0 / (1.0 + np.exp(-raw["opacity_logit"][rows_].astype(np.float64))) * factor
        raw["opacity_logit"][rows_] = np.log(o / (1.0 - o)).astype(np.float32)
    raw["features"] = np.random.default_rng(23).normal(size=(N, 5)).astype(np.float32)
    return raw


def filter_values(case):
    """The filter of a FULL_CASES frame, float32 [N]; None for a case without the filter."""
    return _filter_values_of(FULL_CASES[case]["profile"], FULL_CASES[case]["scale_modifier"]) if FULL_CASES[case]["filter"] else None


@functools.lru_cache(maxsize=None)
def _filter_values_of(profile, scale_modifier):
    """The scene's filter as tests/test_gpu_filter3d.py makes it: observe and finalize (the float32 restatement) of five
    training cameras at this frame's size, scaled by FILTER_SCALE (over the case's scale_modifier, as the scene's scales
    are), every tenth value zero — from row IDENTITY_FROM on, so that few of the IDENTITY rows are among the ones raw_scene
    puts behind the camera (float32 [N])."""
    import filter3d_ref
    from gsrast_amd import filter3d
    rec, max_focal = filter3d.camera_records(filter3d_ref.orbit_cameras(5, width=W, height=H, radius=5.0, seed=6, arc=1.0))
    v = filter3d_ref.finalize_f32(filter3d_ref.observe_f32(_sized_scene(profile, scale_modifier)["xyz"], rec), max_focal)
    v = (v * np.float32(FILTER_SCALE / scale_modifier)).astype(np.float32)
    v[IDENTITY_FROM::10] = 0.0
    v.setflags(write=False)
    return v


def full_weights(case, seed=29):
    """(w [3,H,W], wd [H,W], wf [C,H,W] or None, wa [H,W] or None), float32: weights() for colour and depth (the colour's all
    zeros where the case says so), white noise on the feature map, a smooth field of one sign on the opacity map."""
    c = FULL_CASES[case]
    w, wd = weights()
    rng = np.random.default_rng(seed)
    wf = rng.normal(size=(5, H, W)).astype(np.float32)[:c["channels"]] if c["channels"] else None
    wa = (0.5 + 0.2 * rng.normal(size=(H, W))).astype(np.float32) if c["opacity"] else None
    return (w if c["colour"] else np.zeros_like(w)), wd, wf, wa


def full_row_arrays(case, scales, opacities, means3D, rotations, cam, smoothed=None):
    """The float32 arrays the rasterizer is handed and the row decisions on the way, from the float32 ACTIVATED arrays (the
    restatement's on the CPU, the device's own on the GPU): filter3d_ref.forward_f32, then antialias_ref.compensation_f32.
    smoothed: (scales' [N,4], opacities' [N]) where the caller has the smoothed arrays themselves (the device's): the
    compensation's decisions are then taken on those. Returns dict: scales [N,4], opacities [N] (what gsr_forward reads),
    identity (or None), masks (or None), smoothed (forward_f32's dict or None)."""
    return _row_arrays(FULL_CASES[case], filter_values(case), scales, opacities, means3D, rotations, cam, smoothed)


def _row_arrays(c, filt, scales, opacities, means3D, rotations, cam, smoothed=None):
    import antialias_ref
    import filter3d_ref
    out = dict(scales=np.asarray(scales, np.float32), opacities=np.asarray(opacities, np.float32), identity=None, masks=None, smoothed=None)
    if c["filter"]:
        sm = filter3d_ref.forward_f32(out["scales"], out["opacities"], filt)
        out.update(scales=sm["scales_out"], opacities=sm["opacities_out"], identity=sm["identity"], smoothed=sm)
        if smoothed is not None:
            out.update(scales=np.asarray(smoothed[0], np.float32), opacities=np.asarray(smoothed[1], np.float32))
    if c["antialiased"]:
        m = antialias_ref.compensation_f32(means3D, out["scales"], rotations, out["opacities"], cam.view, cam.proj, cam.tan_fovx,
                                           cam.tan_fovy, W, H, c["profile"], c["scale_modifier"])
        out.update(opacities=m["o_out"], masks=m)
    return out


def full_structure_of(case, cam, rows, radii, ranges, values, n_contrib, clamped=None):
    """The structure of a FULL_CASES frame: structure_of plus the row decisions of full_row_arrays' result `rows`."""
    return R.with_decisions(structure_of(full_scene(case), cam, radii, ranges, values, n_contrib, clamped),
                            rows["masks"], rows["identity"])


def full_forward_options(case, cut=None, **more):
    c = FULL_CASES[case]
    return dict(background=BG, profile=c["profile"], sh_degree=c["sh_degree"], scale_modifier=c["scale_modifier"], depth=c["depth"],
                cut=cut, filter_3d=filter_values(case), antialiased=c["antialiased"],
                opacity=c["opacity"], **more)


def full_leaves(case, dtype=R.F64):
    c = FULL_CASES[case]
    raw = full_scene(case)
    return R.leaves(raw, full_camera_of(case), dtype=dtype, features=raw["features"][:, :c["channels"]] if c["channels"] else None,
                    constant=c["constant"])


def full_reference_step(case, structure, cut=None, dtype=R.F64, drop=None):
    """(grads, color, depth, aux, drop) of a FULL_CASES step on `structure`, as reference_step gives them for CASES."""
    cam = full_camera_of(case)
    w, wd, wf, wa = full_weights(case)
    if drop is None:
        none = np.zeros((H, W), bool)
        aux = R.gradients(full_leaves(case), structure, cam, w, wd, none, wf=wf, wa=wa, **full_forward_options(case))[3]
        drop = R.pixels_to_drop(aux, structure)
    return R.gradients(full_leaves(case, dtype), structure, cam, w, wd, drop, dtype=dtype, wf=wf, wa=wa,
                       **full_forward_options(case, cut)) + (drop,)


# ---- the frames of the geometry regularisers (tests/test_step_geometry_cpu.py, tests/test_gpu_step_geometry.py): the distortion
# map, the normal map with the normal-consistency term, the median map. Same pose, size and scene family as FULL_CASES.
# distortion / median: None, "depth" or "values" (a [N] leaf of the scene); surface: which depth the consistency term's normal is
# taken from ("expected": depth / opacity; "median"), None for no such term; lam_d, lam_n: the weights of the distortion and the
# consistency term, chosen so that each term's share of the largest entry of xyz.grad and of rotation.grad lies between a tenth
# and ten times the colour's (tests/test_step_geometry_cpu.py prints the shares and asserts the band); linear: the maps that
# carry a plain linear weight. constant: the view matrix is no leaf under antialiased=True or normals=True (the library refuses it).
def _geometry(profile, deg, mod=1.0, kx=1.0, depth=False, filt=False, antialiased=False, channels=0, opacity=False, colour=True,
              normals=False, distortion=None, power=2, median=None, threshold=0.5, surface=None, lam_d=1.0, lam_n=1.0, linear=(), wide=1.0):
    return dict(wide=wide, profile=profile, sh_degree=deg, depth=depth, scale_modifier=mod, kx=kx, filter=filt, antialiased=antialiased,
                channels=channels, opacity=opacity, colour=colour, normals=normals, distortion=distortion, power=power, median=median,
                threshold=threshold, surface=surface, lam_d=lam_d, lam_n=lam_n, linear=tuple(linear),
                constant=("view",) if (antialiased or normals) else ())


WIDE_FAINTER = 0.6            # pose-distortion-median: the wide splats' opacity once more multiplied by this — under the upstream profile
                              # they cover the whole frame, and some pixel must blend nothing and select no median id
LAMBDA = {"2dgs-inria": (0.5, 1.0), "2dgs-gscuda-median": (1.0, 1.0)}       # case -> (lam_d, lam_n)
GEOMETRY_CASES = {
    "2dgs-inria": _geometry("inria", 3, depth=True, filt=True, antialiased=True, opacity=True, normals=True, distortion="depth",
                            power=2, surface="expected", lam_d=LAMBDA["2dgs-inria"][0], lam_n=LAMBDA["2dgs-inria"][1]),
    "2dgs-gscuda-median": _geometry("gscuda", 0, mod=2.0, depth=True, opacity=True, normals=True, distortion="depth", power=1,
                                    median="depth", threshold=0.5, surface="median", lam_d=LAMBDA["2dgs-gscuda-median"][0],
                                    lam_n=LAMBDA["2dgs-gscuda-median"][1]),
    "pose-distortion-median": _geometry("inria", 2, kx=1.7, depth=True, distortion="depth", power=2, median="depth",
                                        linear=("depth", "distortion", "median"), wide=WIDE_FAINTER),
    "value-tensors": _geometry("gscuda", 0, channels=2, colour=False, normals=True, distortion="values", power=1, median="values",
                               threshold=0.05, linear=("distortion", "median", "features", "normal_map")),
    "normals-alone": _geometry("inria", 1, filt=True, colour=False, normals=True, linear=("normal_map",)),
}
FLATTEN = (0.3, 0.6)          # one seeded axis of every Gaussian becomes its shortest scale times a factor from this band: the sizes
                              # of full_scene tie two or three scales of many rows (the clips, the stacks), and which axis is the
                              # shortest must be a decision far from its threshold


def geometry_camera_of(case):
    from helpers import posed_camera
    return posed_camera(W, H, kx=GEOMETRY_CASES[case]["kx"], **P1)


@functools.lru_cache(maxsize=None)
def geometry_scene(case):
    """The sizes of full_scene for the case's profile and scale_modifier, copied, every Gaussian flattened along one seeded axis
    (FLATTEN: that axis becomes the row's shortest scale times the factor), plus "distortion_values" and "median_values" [N], standard normal (of either sign, in no order along the lists)."""
    c = GEOMETRY_CASES[case]
    raw = {k: v.copy() for k, v in _sized_scene(c["profile"], c["scale_modifier"]).items()}
    rng = np.random.default_rng(31)
    axis, factor = rng.integers(0, 3, N), rng.uniform(*FLATTEN, N)
    raw["log_scale"][np.arange(N), axis] = raw["log_scale"].min(1) + np.log(factor).astype(np.float32)
    if c["wide"] != 1.0:
        o = 1.0 / (1.0 + np.exp(-raw["opacity_logit"][140:148].astype(np.float64))) * c["wide"]
        raw["opacity_logit"][140:148] = np.log(o / (1.0 - o)).astype(np.float32)
    raw["distortion_values"] = rng.normal(size=N).astype(np.float32)
    raw["median_values"] = rng.normal(size=N).astype(np.float32)
    return raw


def geometry_filter_values(case):
    c = GEOMETRY_CASES[case]
    return _filter_values_of(c["profile"], c["scale_modifier"]) if c["filter"] else None


def geometry_weights(case, seed=37):
    """dict of float32 weights: w [3,H,W] (zeros where the case has no colour term), wf [C,H,W] or None, and for the maps of
    the case g_d, g_m [H,W] (a smooth field of one sign on the distortion map, as a mean over the pixels gives it; white noise
    on the median map) and w_n [3,H,W] (white noise on the normal map, where it carries a linear weight)."""
    c = GEOMETRY_CASES[case]
    w, wd = weights()
    rng = np.random.default_rng(seed)
    wf = rng.normal(size=(5, H, W)).astype(np.float32)[:c["channels"]] if c["channels"] else None
    g_d = (1.0 + 0.25 * rng.normal(size=(H, W))).astype(np.float32)
    g_m = rng.normal(size=(H, W)).astype(np.float32)
    w_n = rng.normal(size=(3, H, W)).astype(np.float32)
    return dict(w=w if c["colour"] else np.zeros_like(w), wd=wd if "depth" in c["linear"] else np.zeros_like(wd), wf=wf, g_d=g_d, g_m=g_m, w_n=w_n)


def geometry_row_arrays(case, scales, opacities, means3D, rotations, cam, smoothed=None):
    """full_row_arrays for a GEOMETRY_CASES frame, plus "normal_decisions": normals_ref.gaussian_normals_f32's decisions on the
    float32 arrays the normals' kernel is handed (the smoothed scales; None for a case without normals)."""
    import normals_ref
    c = GEOMETRY_CASES[case]
    out = _row_arrays(c, geometry_filter_values(case), scales, opacities, means3D, rotations, cam, smoothed)
    out["normal_decisions"] = (normals_ref.gaussian_normals_f32(means3D, out["scales"], rotations, cam.view, c["profile"])[1]
                               if c["normals"] else None)
    return out


def geometry_structure_of(case, cam, rows, radii, ranges, values, n_contrib, clamped=None, median_ids=None):
    """The structure of a GEOMETRY_CASES frame: structure_of, the row decisions of geometry_row_arrays' result `rows`, and the
    median map's ids (median_ref.forward's on the CPU, the device's on the GPU)."""
    s = R.with_decisions(structure_of(geometry_scene(case), cam, radii, ranges, values, n_contrib, clamped), rows["masks"], rows["identity"])
    return R.with_geometry(s, rows["normal_decisions"], median_ids)


def geometry_forward_options(case, cut=None):
    c = GEOMETRY_CASES[case]
    return dict(background=BG, profile=c["profile"], sh_degree=c["sh_degree"], scale_modifier=c["scale_modifier"], depth=c["depth"],
                cut=cut, filter_3d=geometry_filter_values(case), antialiased=c["antialiased"], opacity=c["opacity"],
                distortion=c["distortion"], distortion_power=c["power"], normals=c["normals"], median=c["median"],
                median_threshold=c["threshold"])


def geometry_leaves(case, dtype=R.F64):
    c, raw = GEOMETRY_CASES[case], geometry_scene(case)
    return R.leaves(raw, geometry_camera_of(case), dtype=dtype, features=raw["features"][:, :c["channels"]] if c["channels"] else None,
                    constant=c["constant"], distortion_values=raw["distortion_values"] if c["distortion"] == "values" else None,
                    median_values=raw["median_values"] if c["median"] == "values" else None)


def geometry_loss_terms(case, consistency=None, only=None):
    """step_autograd_ref.gradients' loss_terms of the case. consistency: dict(decisions=, keep_n=) for a case with a consistency
    term (None leaves the term out). only: keep just these terms, for the shares of the terms ("distortion", "consistency", ...)."""
    c, g = GEOMETRY_CASES[case], geometry_weights(case)
    terms = {}
    if c["distortion"]:
        terms["distortion"] = (c["lam_d"], g["g_d"])
    if c["median"] and "median" in c["linear"]:
        terms["median"] = g["g_m"]
    if "normal_map" in c["linear"]:
        terms["normal_map"] = g["w_n"]
    if c["surface"] and consistency is not None:
        terms["consistency"] = dict(weight=c["lam_n"], surface=c["surface"], semantics=c["profile"], **consistency)
    return terms if only is None else {k: v for k, v in terms.items() if k in only}


def surface_of(case, depth, opacity_map, median_map):
    """The image the consistency term's depth normal reads, in the arrays' own type (numpy): depth / max(opacity, 1e-6), or the
    median map."""
    if GEOMETRY_CASES[case]["surface"] == "median":
        return median_map
    return depth / np.maximum(opacity_map, opacity_map.dtype.type(1e-6))


def geometry_reference_step(case, structure, surface32=None, cut=None, dtype=R.F64, drop=None, keep_n=None, only=None, colour=True):
    """(grads, color, depth, aux, drop, keep_n) of a GEOMETRY_CASES step on `structure`. surface32: the float32 image the library's
    depth normals read (surface_of of the float32 maps — the CPU oracle's or the device's), for a case with a consistency term.
    drop, keep_n: None — decided here by the uncut float64 forward (step_autograd_ref.pixels_to_drop, consistency_pixels).
    only: the loss terms kept (geometry_loss_terms); colour=False: without the colour term — for the shares of the terms."""
    import normals_ref
    c, cam, g = GEOMETRY_CASES[case], geometry_camera_of(case), geometry_weights(case)
    w = g["w"] if colour else np.zeros_like(g["w"])
    wf = g["wf"] if (only is None or "features" in only) else None
    tan = (cam.tan_fovx, cam.tan_fovy)
    decisions = normals_ref.depth_normals_f32(surface32, tan, c["profile"])[1] if c["surface"] else None
    if drop is None:
        none = np.zeros((H, W), bool)
        _, _, dmap, aux = R.gradients(geometry_leaves(case), structure, cam, w, g["wd"], none, wf=wf,
                                      loss_terms=geometry_loss_terms(case), **geometry_forward_options(case))
        drop = R.pixels_to_drop(aux, structure)
        if c["surface"]:
            keep_n = R.consistency_pixels(drop, surface_of(case, dmap, aux["opacity_map"], aux.get("median_map")), tan, c["profile"], decisions)
    consistency = dict(decisions=decisions, keep_n=keep_n) if c["surface"] else None
    return R.gradients(geometry_leaves(case, dtype), structure, cam, w, g["wd"], drop, dtype=dtype, wf=wf,
                       loss_terms=geometry_loss_terms(case, consistency, only), **geometry_forward_options(case, cut)) + (drop, keep_n)


def weights(seed=17):
    """The loss weights (float32 numpy): white noise on the colour; on the depth a smooth field of one sign, as a depth loss
    gives it (tests/test_gpu_backward_poses.py, the depth term)."""
    rng = np.random.default_rng(seed)
    return rng.normal(size=(3, H, W)).astype(np.float32), (1.0 + 0.25 * rng.normal(size=(H, W))).astype(np.float32)


def activated_scene(raw):
    """The arrays gsr_forward takes, in the float32 arithmetic of csrc/activation_math.hpp (numpy; the exponential is libm's
    there and numpy's here: the CPU oracles are run on these, the GPU on its own)."""
    f = np.float32
    n = raw["xyz"].shape[0]
    r = raw["rotation"].astype(f)
    d = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + (r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])
    inv = f(1.0) / np.sqrt(d)
    return {"means3D": np.concatenate([raw["xyz"].astype(f), np.ones((n, 1), f)], 1),
            "scales": np.concatenate([np.exp(raw["log_scale"].astype(f)), np.full((n, 1), np.exp(f(1.0)), f)], 1).astype(f),
            "rotations": (r * inv[:, None]).astype(f),
            "opacities": (f(1.0) / (f(1.0) + np.exp(-raw["opacity_logit"].astype(f)))).astype(f),
            "shs": raw["shs"].astype(f)}


def structure_of(raw, cam, radii, ranges, values, n_contrib, clamped=None):
    """step_autograd_ref.structure_of for a frame of this module, from a forward state's arrays."""
    return R.structure_of(raw["xyz"], cam.view, cam.tan_fovx, cam.tan_fovy, W, H, radii, ranges, values, n_contrib, clamped)


def forward_options(case, cut=None):
    profile, deg, depth, mod, _, _ = CASES[case]
    return dict(background=BG, profile=profile, sh_degree=deg, scale_modifier=mod, depth=depth, cut=cut)


def reference_step(raw, cam, case, structure, w, wd, cut=None, dtype=R.F64, drop=None):
    """(grads, color, depth, aux, drop) of the case's step on `structure` (step_autograd_ref.gradients). drop: the pixels
    left out; None: decided here, by the uncut float64 forward (step_autograd_ref.pixels_to_drop)."""
    precomp = CASES[case][5]
    if drop is None:
        none = np.zeros((H, W), bool)
        aux = R.gradients(R.leaves(raw, cam, colors=precomp), structure, cam, w, wd, none, **forward_options(case))[3]
        drop = R.pixels_to_drop(aux, structure)
    leaf = R.leaves(raw, cam, dtype=dtype, colors=precomp)
    return R.gradients(leaf, structure, cam, w, wd, drop, dtype=dtype, **forward_options(case, cut)) + (drop,)
