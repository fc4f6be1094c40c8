"""GPU: one training step through everything autograd.render composes — the 3D smoothing filter, the opacity compensation of
antialiased=True, the feature map, the differentiable opacity map, colour and depth — against the float64 autograd reference
of the same step (tests/step_autograd_ref.py with its options on: one graph from the raw parameters to the loss, in the order
`render` documents, differentiated by torch.autograd, on the structure and the float32 row decisions read back from the device).
Nothing is stitched from the rasterizer's own leaf gradients: the order of modifier and filter, the scales the compensation
reads under the filter, whether c's gradient is added to the rasterizer's, whether the feature term reaches o' and from there c
and the filter, are in the reference because they are in its forward.

Compared: every raw parameter's gradient, the features', every camera leaf's, FrameSlot.dL_dmean2D, and the four maps. The
frames (tests/step_frames.py, FULL_CASES), their conditions, the bounds (the float32 noise floor), the cuts and the caps are
tests/test_step_full_cpu.py's, which needs no GPU. The two caps are asserted again here, on the device's own arrays."""
import numpy as np
import pytest

import step_autograd_ref as R
import step_frames as S
from camera_grad_ref import ZERO_ENTRIES
from step_frames import BG, FULL_CASES, H, N, RAW, W

pytestmark = pytest.mark.gpu

DRAW = dict(plan="sort", tile_history=False)
CAMERA = ("view", "proj", "cam_pos")


def _step(case, draw):
    """The case's step on the GPU and its reference: dict of got / want (gradients keyed by array name), the maps, the
    structure, the dropped pixels, the reference's aux and the rasterizer."""
    import torch
    from gsrast_amd import filter3d
    from gsrast_amd.autograd import FrameSlot, GaussianParams, activate, render
    from gsrast_amd.rasterizer import SplatRasterizer
    from test_gpu_backward_poses import _state
    c = FULL_CASES[case]
    raw, cam = S.full_scene(case), S.full_camera_of(case)
    dev = torch.device("cuda:0")
    tensor = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(dev)
    camera = {k: tensor(getattr(cam, k)).requires_grad_(k not in c["constant"]) for k in CAMERA}
    params = GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if c["profile"] == "inria" else "file",
                                     device=dev)
    feats = tensor(raw["features"][:, :c["channels"]]).requires_grad_(True) if c["channels"] else None
    filt = tensor(S.filter_values(case)) if c["filter"] else None
    rast, slot = SplatRasterizer(W, H, background=BG), FrameSlot()
    out = render(params, rast, (camera["view"], camera["proj"], camera["cam_pos"], cam.tan_fovx, cam.tan_fovy),
                 semantics=c["profile"], sh_degree=c["sh_degree"], scale_modifier=c["scale_modifier"], depth=c["depth"],
                 radii_slot=slot, opacity_grad=c["opacity"], antialiased=c["antialiased"], filter_3d=filt, features=feats, **draw)
    color, dmap, omap = out[:3]
    fmap = out[3] if feats is not None else None
    # the structure of the frame the rasterizer holds, and the float32 arrays the row decisions are taken from (read back
    # before the backward: nothing draws in between)
    g, im, plist, clamped = _state(rast)
    with torch.no_grad():
        act = activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
        smoothed = filter3d.smoothed(act[1], act[3], filt) if c["filter"] else None
    host = lambda t: t.cpu().numpy()
    rows = S.full_row_arrays(case, host(act[1]), host(act[3]), host(act[0]), host(act[2]), cam,
                             smoothed=(host(smoothed[0]), host(smoothed[1])) if smoothed is not None else None)
    structure = S.full_structure_of(case, cam, rows, g["radii"], im["ranges"], plist, im["nContrib"],
                                    clamped if c["profile"] == "inria" else None)
    want, ref_color, ref_depth, aux, drop = S.full_reference_step(case, structure)
    w, wd, wf, wa = S.full_weights(case)
    keep = torch.from_numpy(~drop).to(dev)
    loss = (tensor(w) * keep * color).sum()
    if c["depth"]:
        loss = loss + (tensor(wd) * keep * dmap).sum()
    if c["opacity"]:
        loss = loss + (tensor(wa) * keep * omap).sum()
    if feats is not None:
        loss = loss + (tensor(wf) * keep * fmap).sum()
    loss.backward()
    torch.cuda.synchronize()
    tensors = {k: getattr(params, k) for k in RAW}
    if feats is not None:
        tensors["features"] = feats
    tensors.update({k: t for k, t in camera.items() if t.requires_grad})
    got = {k: t.grad.detach().cpu().numpy().astype(np.float64) for k, t in tensors.items()}
    vis = aux["visible"]
    got["mean2D"] = slot.dL_dmean2D.detach().cpu().numpy().astype(np.float64)
    want = dict(want, mean2D=np.zeros((N, 2)))
    want["mean2D"][vis] = want["per_gaussian.mean2D"]
    maps = {"color": (host(color.detach()), ref_color), "depth": (host(dmap.detach()), ref_depth) if c["depth"] else None,
            "opacity": (host(omap.detach()), aux["opacity_map"]) if c["opacity"] else None,
            "features": (host(fmap.detach()), aux["feature_map"]) if feats is not None else None}
    return dict(got=got, want=want, maps=maps, structure=structure, drop=drop, aux=aux, rast=rast, cam=cam)


def _assert_bounds(case, got, want, what):
    """Every array within its bound of the reference's largest entry; returns the worst error as a share of its bound."""
    worst = 0.0
    for k, a in got.items():
        ref = want[k].reshape(a.shape)
        assert np.isfinite(a).all(), (what, k)
        scale = float(np.abs(ref).max())
        if scale == 0:                                           # (the gscuda profile does not read cam_pos; no colour weight: shs)
            assert (a == 0).all(), (what, k)
            continue
        err = float(np.abs(a - ref).max()) / scale
        b = R.bound(case, k)
        print(f"[step full] {what}: {k}.grad worst error {err:.3e} of the largest entry = {err / b:.3f} of the bound")
        assert err <= b, (what, k, err, b)
        worst = max(worst, err / b)
    print(f"[step full] {what}: worst array at {worst:.3f} of its bound")
    return worst


def _assert_caps(case, s):
    """At most 1 % of the pixels dropped; no Gaussian row near a threshold of the compensation or the smoothing, and the
    float64 decisions are the device arrays' float32 ones."""
    c = FULL_CASES[case]
    assert s["drop"].sum() <= 0.01 * W * H, int(s["drop"].sum())
    near, differ = R.rows_near_a_threshold(s["aux"], s["structure"], s["cam"].tan_fovx, s["cam"].tan_fovy, S.filter_values(case),
                                           c["antialiased"])
    assert not near.any() and not differ.any(), (case, np.nonzero(near)[0], np.nonzero(differ)[0])


@pytest.mark.parametrize("case", list(FULL_CASES))
def test_full_step_gradients_match_the_float64_autograd_reference(case):
    from helpers import image_report
    c = FULL_CASES[case]
    s = _step(case, DRAW)
    got, want, structure, aux = s["got"], s["want"], s["structure"], s["aux"]
    vis = structure["vis"]
    assert vis.sum() >= N / 2 and (~vis).sum() >= N / 8
    _assert_caps(case, s)
    _assert_bounds(case, got, want, case)
    # exact zeros: the culled rows of every per-Gaussian array, the feature rows of Gaussians no pixel composites, the camera
    # entries no path reaches
    for k, a in got.items():
        if k not in CAMERA:
            assert (a[~vis] == 0).all(), (case, k)
    if c["channels"]:
        idle = aux["visible"][~aux["blended"]]
        print(f"[step full] {case}: {idle.size} visible Gaussians blend nothing")
        assert idle.size > 0 and (got["features"][idle] == 0).all(), case
    cam35 = np.concatenate([got[k].reshape(-1) if k in got else np.zeros(n) for k, n in zip(CAMERA, (16, 16, 3))])
    assert (cam35[ZERO_ENTRIES] == 0).all(), case
    keep = ~s["drop"]
    for name, pair in s["maps"].items():
        if pair is None:
            continue
        worst, bad, _ = image_report(pair[0] * keep, pair[1] * keep)
        print(f"[step full] {case}: {name} map worst {worst:.3e}, {int(s['drop'].sum())} pixels dropped")
        assert bad == 0, (case, name, worst)


def test_full_step_gradients_through_the_block_list_feed():
    """The upstream case with everything on again with plan="blocks": the blend, the render backward and the feature passes
    are fed by the block lists. Only the bounds are asserted: the other plan's bits are tests/test_gpu_backward_blocks.py's."""
    case = "full-inria"
    s = _step(case, dict(plan="blocks", overlap_emit=True, tile_history=False))
    assert s["rast"].last_plan == "blocks" and s["rast"].last_lists_written
    _assert_caps(case, s)
    _assert_bounds(case, s["got"], s["want"], case + ", block lists")
