"""The frames of the training-step tests (tests/test_step_autograd_cpu.py, tests/test_gpu_step_autograd.py): the cases, the
scene in raw parameters, the camera, the loss weights, and the reference step of a case (tests/step_autograd_ref.py)."""
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
