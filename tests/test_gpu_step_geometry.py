"""GPU: one training step through autograd.render with the three geometry regularisers composed around the rasterizer — the
distortion map, the normal map with normals.normal_consistency (over the expected depth, or the median depth as surface_depth),
the median map — against the float64 autograd reference of the same step (tests/step_autograd_ref.py with those options on: one
graph from the raw parameters to the loss, differentiated by torch.autograd, on the structure, the float32 row decisions, the
depth normals' decisions and the median ids read back from the device). Nothing is stitched from the kernels' own leaf gradients:
whether the distortion seed reaches c and the filter's coefficient, whether the normal channels' gradient slice lands on its own
columns behind the caller's features, whether the camera receives both the kernel's path and torch's path through z, whether
the opacity map is a constant of the depth normal's weight, are in the reference because they are in its forward.

Compared: every raw parameter's gradient, the value tensors', the features', every camera leaf's, FrameSlot.dL_dmean2D, and every
map. The frames (tests/step_frames.py, GEOMETRY_CASES), their conditions, the bounds (the float32 noise floor), the cuts and the
caps are tests/test_step_geometry_cpu.py's, which needs no GPU. The caps are asserted again here, on the device's own arrays."""
import numpy as np
import pytest

import step_autograd_ref as R
import step_frames as S
from camera_grad_ref import ZERO_ENTRIES
from step_frames import BG, GEOMETRY_CASES, H, N, RAW, W

pytestmark = pytest.mark.gpu

DRAW = dict(plan="sort", tile_history=False)
CAMERA = ("view", "proj", "cam_pos")


def _step(case, draw):
    """The case's step on the GPU and its reference: dict of got / want (gradients keyed by array name), the maps, the
    structure, the dropped pixels and the ones without the consistency term, the reference's aux and the rasterizer."""
    import torch
    import normals_ref
    from gsrast_amd import filter3d, normals
    from gsrast_amd.autograd import FrameSlot, GaussianParams, activate, render
    from gsrast_amd.rasterizer import SplatRasterizer
    from test_gpu_backward_poses import _state
    c = GEOMETRY_CASES[case]
    raw, cam = S.geometry_scene(case), S.geometry_camera_of(case)
    tan = (cam.tan_fovx, cam.tan_fovy)
    dev = torch.device("cuda:0")
    tensor = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(dev)
    camera = {k: tensor(getattr(cam, k)).requires_grad_(k not in c["constant"]) for k in CAMERA}
    params = GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if c["profile"] == "inria" else "file",
                                     device=dev)
    feats = tensor(raw["features"][:, :c["channels"]]).requires_grad_(True) if c["channels"] else None
    values = {k: tensor(raw[k + "_values"]).requires_grad_(True) for k in ("distortion", "median") if c[k] == "values"}
    filt = tensor(S.geometry_filter_values(case)) if c["filter"] else None
    rast, slot = SplatRasterizer(W, H, background=BG), FrameSlot()
    out = render(params, rast, (camera["view"], camera["proj"], camera["cam_pos"], cam.tan_fovx, cam.tan_fovy),
                 semantics=c["profile"], sh_degree=c["sh_degree"], scale_modifier=c["scale_modifier"], depth=c["depth"],
                 radii_slot=slot, opacity_grad=c["opacity"], antialiased=c["antialiased"], filter_3d=filt, features=feats,
                 distortion=values.get("distortion", c["distortion"]), distortion_power=c["power"], normals=c["normals"],
                 median=values.get("median", c["median"]), median_threshold=c["threshold"], **draw)
    # (color, depth, opacity_map[, feature_map][, normal_map][, distortion_map][, median_map])
    rest = list(out[3:])
    color, dmap, omap = out[:3]
    fmap = rest.pop(0) if feats is not None else None
    nmap = rest.pop(0) if c["normals"] else None
    dist = rest.pop(0) if c["distortion"] else None
    med = rest.pop(0) if c["median"] else None
    assert not rest
    # the structure of the frame the rasterizer holds, the float32 arrays the row decisions are taken from, the maps the depth
    # normals read and the median ids (read back before the backward: nothing draws in between)
    host = lambda t: t.detach().cpu().numpy()
    g, im, plist, clamped = _state(rast)
    with torch.no_grad():
        act = activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
        smoothed = filter3d.smoothed(act[1], act[3], filt) if c["filter"] else None
        surface = None
        if c["surface"]:
            surface = host(med if c["surface"] == "median" else dmap / omap.clamp_min(1e-6))
        ids = None
        if c["median"]:
            v = camera["view"].reshape(-1)
            z = (act[0][:, 0] * v[2] + act[0][:, 1] * v[6]) + (act[0][:, 2] * v[10] + v[14])        # (as autograd.rasterize forms "depth")
            again = rast.render_median(values["median"].detach() if "median" in values else z, threshold=c["threshold"], ids=True, sync=False)
            held = med.grad_fn.ids                                # (what _Median holds for its backward)
            assert held.dtype == torch.int32 and torch.equal(held, again["ids"]), case
            assert torch.equal(again["map"].view(torch.int32), med.detach().view(torch.int32)), case
            ids = host(held)
    rows = S.geometry_row_arrays(case, host(act[1]), host(act[3]), host(act[0]), host(act[2]), cam,
                                 smoothed=(host(smoothed[0]), host(smoothed[1])) if smoothed is not None else None)
    structure = S.geometry_structure_of(case, cam, rows, g["radii"], im["ranges"], plist, im["nContrib"],
                                        clamped if c["profile"] == "inria" else None, ids)
    want, ref_color, ref_depth, aux, drop, keep_n = S.geometry_reference_step(case, structure, surface)
    wts = S.geometry_weights(case)
    keep = torch.from_numpy(~drop).to(dev)
    loss = (tensor(wts["w"]) * keep * color).sum()
    if "depth" in c["linear"]:
        loss = loss + (tensor(wts["wd"]) * keep * dmap).sum()
    if feats is not None:
        loss = loss + (tensor(wts["wf"]) * keep * fmap).sum()
    if c["distortion"]:
        loss = loss + c["lam_d"] * (tensor(wts["g_d"]) * keep * dist).sum()
    if "median" in c["linear"]:
        loss = loss + (tensor(wts["g_m"]) * keep * med).sum()
    if "normal_map" in c["linear"]:
        loss = loss + (tensor(wts["w_n"]) * keep * nmap).sum()
    if c["surface"]:
        term = normals.normal_consistency(nmap, dmap, omap, tan, semantics=c["profile"],
                                          surface_depth=med if c["surface"] == "median" else None)
        loss = loss + c["lam_n"] * (torch.from_numpy(keep_n).to(dev) * term).sum()
    loss.backward()
    torch.cuda.synchronize()
    tensors = {k: getattr(params, k) for k in RAW}
    if feats is not None:
        tensors["features"] = feats
    tensors.update({k + "_values": t for k, t in values.items()})
    tensors.update({k: t for k, t in camera.items() if t.requires_grad})
    got = {k: t.grad.detach().cpu().numpy().astype(np.float64) for k, t in tensors.items()}
    got["mean2D"] = slot.dL_dmean2D.detach().cpu().numpy().astype(np.float64)
    want = dict(want, mean2D=np.zeros((N, 2)))
    want["mean2D"][aux["visible"]] = want["per_gaussian.mean2D"]
    pair = lambda t, ref: (host(t), ref) if t is not None else None
    maps = {"color": (host(color), ref_color), "depth": pair(dmap if c["depth"] else None, ref_depth),
            "opacity": pair(omap if c["opacity"] else None, aux["opacity_map"]), "features": pair(fmap, aux["feature_map"]),
            "normals": pair(nmap, aux.get("normal_map")), "distortion": pair(dist, aux.get("distortion_map")),
            "median": pair(med, aux.get("median_map"))}
    surface_normal = normals_ref.depth_normals_f32(surface, tan, c["profile"])[0] if c["surface"] else None
    return dict(got=got, want=want, maps=maps, structure=structure, drop=drop, keep_n=keep_n, aux=aux, rast=rast, cam=cam,
                surface_normal=surface_normal)


def _assert_bounds(case, got, want, what):
    """Every array within its bound of the reference's largest entry; returns the worst error as a share of its bound."""
    worst = (0.0, None)
    for k, a in got.items():
        ref = want[k].reshape(a.shape)
        assert np.isfinite(a).all(), (what, k)
        scale = float(np.abs(ref).max())
        if scale == 0:                                           # (the gscuda profile does not read cam_pos; no colour weight: shs)
            assert (a == 0).all(), (what, k)
            continue
        err = float(np.abs(a - ref).max()) / scale
        b = R.bound(case, k)
        print(f"[step geometry] {what}: {k}.grad worst error {err:.3e} of the largest entry = {err / b:.3f} of the bound")
        assert err <= b, (what, k, err, b)
        if err / b >= worst[0]:
            worst = (err / b, k)
    return worst


def _assert_caps(case, s, what):
    from test_step_geometry_cpu import assert_caps
    dropped, lost = assert_caps(case, s["drop"], s["keep_n"], s["aux"], s["structure"], s["cam"], s["surface_normal"])
    return f"{dropped} pixels dropped, {lost} more without the consistency term"


@pytest.mark.parametrize("case", list(GEOMETRY_CASES))
def test_geometry_step_gradients_match_the_float64_autograd_reference(case):
    from helpers import image_report
    s = _step(case, DRAW)
    got, structure = s["got"], s["structure"]
    vis = structure["vis"]
    assert vis.sum() >= N / 2 and (~vis).sum() >= N / 8
    pixels = _assert_caps(case, s, case)
    worst = _assert_bounds(case, got, s["want"], case)
    print(f"[step geometry] {case}: worst array {worst[1]} at {worst[0]:.3f} of its bound; {pixels}")
    # exact zeros: the culled rows of every per-Gaussian array, the camera entries no path reaches
    for k, a in got.items():
        if k not in CAMERA:
            assert (a[~vis] == 0).all(), (case, k)
    cam35 = np.concatenate([got[k].reshape(-1) if k in got else np.zeros(n) for k, n in zip(CAMERA, (16, 16, 3))])
    assert (cam35[ZERO_ENTRIES] == 0).all(), case
    keep = ~s["drop"]
    for name, pair in s["maps"].items():
        if pair is None:
            continue
        worst_px, bad, _ = image_report(pair[0] * keep, pair[1] * keep)
        print(f"[step geometry] {case}: {name} map worst {worst_px:.3e}")
        assert bad == 0, (case, name, worst_px)
    if GEOMETRY_CASES[case]["median"]:                           # the ids: equal wherever the pixel is not dropped
        assert ((s["aux"]["median_selected"] == structure["median_ids"]) | s["drop"]).all(), case


def test_geometry_step_gradients_through_the_block_list_feed():
    """The upstream 2DGS case again with plan="blocks": the list walks (features with the normals, distortion) read the sorted
    lists while the blend and the render backward are fed by the block lists. Only the bounds are asserted."""
    case = "2dgs-inria"
    s = _step(case, dict(plan="blocks", overlap_emit=True, tile_history=False))
    assert s["rast"].last_plan == "blocks"
    pixels = _assert_caps(case, s, case)
    worst = _assert_bounds(case, s["got"], s["want"], case + ", block lists")
    print(f"[step geometry] {case}, block lists: worst array {worst[1]} at {worst[0]:.3f} of its bound; {pixels}")
