"""GPU: one training step — `render(params, rast, camera_tuple)`, a loss on colour and depth, `loss.backward()` — against the
float64 autograd reference of the same step (tests/step_autograd_ref.py: the forward restated in plain torch, differentiated
by torch.autograd, on the structure read back from the same rasterizer). All five parameters and the three camera tensors
require gradients. Nothing here is derived by hand: a coupling that the kernels and the other tests' stitching both lack —
the mean through the Jacobian, cam_pos through the view direction, the depth channel to the mean, scale_modifier into the
scale gradient — is in the reference because it is in the forward.

Frames: 40 x 24 pixels (3 x 2 tiles, ragged on both edges), 150 Gaussians (two whole waves and a partial one), pose P1 of
tests/test_gpu_backward_poses.py (tests/step_frames.py); the scene's conditions, the reference's pin to the CPU oracles,
the bounds (the float32 noise floor) and the blindness guards (the cuts) are tests/test_step_autograd_cpu.py's, which
needs no GPU."""
import numpy as np
import pytest

import step_autograd_ref as R
import step_frames as S
from camera_grad_ref import ZERO_ENTRIES
from step_frames import BG, CASES, H, N, RAW, W

pytestmark = pytest.mark.gpu

DRAW = dict(plan="sort", tile_history=False)


def _state(rast):
    from test_gpu_backward_poses import _state as state
    return state(rast)


def _step(case, draw):
    """The case's step on the GPU and its reference. Returns (got, want, drop, images): the gradients keyed by array name."""
    import torch
    from gsrast_amd.autograd import GaussianParams, activate, rasterize, render
    from gsrast_amd.rasterizer import SplatRasterizer
    profile, deg, depth, mod, kx, precomp = CASES[case]
    raw, cam = S.raw_scene(profile), S.camera_of(case)
    dev = torch.device("cuda:0")
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(dev).requires_grad_(True)
    view, proj, pos = leaf(cam.view), leaf(cam.proj), leaf(cam.cam_pos)
    rast = SplatRasterizer(W, H, background=BG)
    if precomp:
        p = {k: leaf(raw[k]) for k in RAW[:4]}
        colors = leaf(raw["colors"])
        act = activate(p["xyz"], p["opacity_logit"], p["log_scale"], p["rotation"])
        shs = torch.from_numpy(raw["shs"]).to(dev)
        color, dmap, _ = rasterize(rast, *act, shs, view, proj, pos, (cam.tan_fovx, cam.tan_fovy), semantics=profile, sh_degree=deg,
                                   scale_modifier=mod, depth=depth, colors_precomp=colors, **draw)
        tensors = dict(p, colors=colors)
    else:
        params = GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if profile == "inria" else "file",
                                         device=dev)
        color, dmap, _ = render(params, rast, (view, proj, pos, cam.tan_fovx, cam.tan_fovy), semantics=profile, sh_degree=deg,
                                scale_modifier=mod, depth=depth, **draw)
        tensors = {k: getattr(params, k) for k in RAW}
    tensors.update(view=view, proj=proj, cam_pos=pos)
    # the structure of the frame the rasterizer holds (read back before the backward: nothing draws in between)
    g, im, plist, clamped = _state(rast)
    structure = S.structure_of(raw, cam, g["radii"], im["ranges"], plist, im["nContrib"],
                               clamped if profile == "inria" and not precomp else None)
    w, wd = S.weights()
    want, ref_color, ref_depth, aux, drop = S.reference_step(raw, cam, case, structure, w, wd)
    keep = torch.from_numpy(~drop).to(dev)
    loss = (torch.from_numpy(w).to(dev) * keep * color).sum()
    if depth:
        loss = loss + (torch.from_numpy(wd).to(dev) * keep * dmap).sum()
    loss.backward()
    torch.cuda.synchronize()
    got = {k: t.grad.detach().cpu().numpy().astype(np.float64) for k, t in tensors.items()}
    images = dict(color=color.detach().cpu().numpy(), depth=dmap.detach().cpu().numpy() if depth else None, ref_color=ref_color,
                  ref_depth=ref_depth)
    return got, want, drop, images, structure, rast


def _assert_bounds(case, got, want, what):
    for k, a in got.items():
        ref = want[k].reshape(a.shape)
        scale = float(np.abs(ref).max())
        if scale == 0:                                           # (the reference's profile does not read cam_pos)
            assert (a == 0).all(), (what, k)
            continue
        err = float(np.abs(a - ref).max()) / scale
        b = R.bound(case, k)
        print(f"[step autograd] {what}: {k}.grad worst error {err:.3e} of the largest entry = {err / b:.3f} of the bound")
        assert np.isfinite(a).all() and err <= b, (what, k, err, b)


@pytest.mark.parametrize("case", list(CASES))
def test_step_gradients_match_the_float64_autograd_reference(case):
    from helpers import image_report
    got, want, drop, images, structure, _ = _step(case, DRAW)
    assert drop.sum() <= 0.01 * W * H, int(drop.sum())
    assert structure["vis"].sum() >= N / 2 and (~structure["vis"]).sum() >= N / 8
    _assert_bounds(case, got, want, case)
    culled = ~structure["vis"]
    for k, a in got.items():
        if k not in ("view", "proj", "cam_pos"):
            assert (a[culled] == 0).all(), (case, k)
    cam35 = np.concatenate([got["view"].reshape(-1), got["proj"].reshape(-1), got["cam_pos"].reshape(-1)])
    assert (cam35[ZERO_ENTRIES] == 0).all(), case
    keep = ~drop
    worst, bad, _ = image_report(images["color"] * keep, images["ref_color"] * keep)
    print(f"[step autograd] {case}: image worst {worst:.3e}, {int(drop.sum())} pixels dropped")
    assert bad == 0, (case, worst)
    if images["depth"] is not None:
        worst_d, bad_d, _ = image_report(images["depth"] * keep, images["ref_depth"] * keep)
        print(f"[step autograd] {case}: depth worst {worst_d:.3e}")
        assert bad_d == 0, (case, worst_d)


def test_step_gradients_through_the_block_list_feed():
    """The first upstream case again with plan="blocks": the blend and the render backward are fed by the block lists (the
    sorted lists are written beside them, for the structure). Only the bound is asserted: the other plan's bits are
    tests/test_gpu_backward_blocks.py's business."""
    case = "inria-3-depth"
    got, want, drop, _, _, rast = _step(case, dict(plan="blocks", overlap_emit=True, tile_history=False))
    assert rast.last_plan == "blocks" and not rast.last_blend_from_lists and rast.last_lists_written
    assert drop.sum() <= 0.01 * W * H
    _assert_bounds(case, got, want, case + ", block lists")
