"""CPU: the float64 autograd reference of the training step (tests/step_autograd_ref.py) with the options autograd.render has
gained since — the 3D smoothing filter, the opacity compensation of antialiased=True, a feature map, the opacity map — on the
frames of tests/test_gpu_step_full.py (tests/step_frames.py, FULL_CASES). As tests/test_step_autograd_cpu.py does for colour
and depth: the forward pinned to the CPU oracles, the float32 noise floor that sets the GPU test's bounds, the cuts (blindness
guards), the conditions on the frames and the caps. No GPU, no library kernel: the structure is the CPU oracles', run on the
float32 restatements of the smoothing (filter3d_ref.forward_f32) and of the compensation (antialias_ref.compensation_f32).

Measured figures (this file prints them; `pytest -s`), as shares of an array's largest entry (images: absolute, per pixel).

1. The forward (no frame drops a pixel; no Gaussian row is near a threshold):
  case                 image    finalT   depth    features opacity
  full-inria           2.8e-7   3.0e-7   1.0e-6   8.0e-7   3.0e-7
  full-gscuda-m2       2.9e-7   3.0e-7   1.0e-7   8.0e-7   3.0e-7
  filter-features-kx   3.3e-7   4.4e-7   1.3e-7   1.0e-6   4.4e-7
  antialias-alone      6.4e-7   6.7e-7   2.6e-6   -        -
  filter-alone         3.1e-7   3.8e-7   1.7e-6   -        -
  features-alone       8.7e-7   1.0e-6   -        1.4e-6   -

2. e32, the float32 restatement against the float64 one (with the square root over the floor and the smoothing in the chain):
  case               xyz     op_logit log_sc. rotation shs     features view    proj    cam_pos mean2D
  full-inria         1.9e-6  1.5e-7  4.1e-7  9.0e-7  9.5e-7  1.1e-6   const   1.6e-6  7.7e-7  1.7e-6
  full-gscuda-m2     4.6e-7  4.5e-7  7.6e-7  2.7e-6  3.4e-7  7.6e-7   const   9.3e-7  -       5.5e-7
  filter-features-kx 2.1e-6  1.3e-7  7.7e-7  1.7e-6  7.5e-7  1.5e-6   1.1e-7  2.1e-6  6.2e-7  3.5e-6
  antialias-alone    1.7e-6  5.3e-7  2.2e-6  3.8e-6  4.5e-7  -        const   4.3e-7  -       1.6e-6
  filter-alone       1.7e-6  9.6e-8  3.9e-7  1.2e-6  4.8e-7  -        2.4e-7  4.4e-7  2.2e-7  2.0e-6
  features-alone     2.1e-6  6.5e-7  3.0e-6  8.6e-7  0       1.0e-6   1.8e-6  5.1e-6  -       3.0e-6
(const: the view matrix is no leaf under antialiased=True; -: the gscuda profile does not read cam_pos; mean2D: the gradient
by the pixel-space centres, FrameSlot.dL_dmean2D.) The square root over the floor and the smoothing add nothing to speak of:
2 e32 stays below 2e-4 everywhere, every GPU bound is at the floor and BOUNDS stays empty (on the GPU the worst array sits at
2.9e-6, tests/test_gpu_step_full.py).

3. The cuts: every new one moves at least one gradient array by more than 100 bounds on every case it applies to. The
smallest over those cases, in bounds (2e-4 of the array's largest entry):
  filter_scale 677 (log_scale), filter_opacity 1753 (opacity_logit), filter_coef 1978 (log_scale), compensation 1615
  (rotation), compensation_scales 138 (log_scale), feature_geometry 3543, opacity_map 656
compensation_scales is the narrow one: what it changes is the product of (1 - s / s') and the share of the scale's gradient that
runs through c, and both are large only on splats of a pixel's size under a filter of that size. The frames' sizes are chosen
so that those are the Gaussians with the largest gradients (tests/step_frames.py; on raw_scene's own sizes the cut moves
log_scale by one bound). The modifier applied before the smoothing moves the colour image of full-gscuda-m2 by 0.16 (423
pixels over the tolerance of 1e-4).
"""
import functools

import numpy as np
import pytest

import step_autograd_ref as R
import step_frames as S
from step_frames import BG, FULL_CASES, H, N, W

IMAGE_TOL = 1e-4                 # helpers.image_report's, what test_restated_forward_is_the_oracles asserts


def _arrays(case):
    c = FULL_CASES[case]
    cam = tuple(k for k in ("view", "proj", "cam_pos") if k not in c["constant"])
    return ("xyz", "opacity_logit", "log_scale", "rotation", "shs") + (("features",) if c["channels"] else ()) + cam


@functools.lru_cache(maxsize=None)
def frame(case):
    """The case's frame on the CPU: the float32 arrays the oracle is fed, the oracle's forward state, the structure with the
    row decisions, and the float64 reference step."""
    from oracle import cpu_oracle, inria_np
    c = FULL_CASES[case]
    raw, cam = S.full_scene(case), S.full_camera_of(case)
    act = S.activated_scene(raw)
    rows = S.full_row_arrays(case, act["scales"], act["opacities"], act["means3D"], act["rotations"], cam)
    scene = dict(act, scales=rows["scales"], opacities=rows["opacities"])
    if c["profile"] == "inria":
        st = inria_np.forward(scene, cam, BG, deg=c["sh_degree"], scale_modifier=c["scale_modifier"], blend_with="numpy-expf")
    else:
        st = cpu_oracle.forward(scene, cam, BG, scale_modifier=c["scale_modifier"])
    structure = S.full_structure_of(case, cam, rows, st["radii"], st["ranges"], st["values"], st["nContrib"], st.get("clamped"))
    grads, color, dmap, aux, drop = S.full_reference_step(case, structure)
    return dict(case=case, raw=raw, cam=cam, scene=scene, act=act, rows=rows, st=st, structure=structure, drop=drop, grads=grads,
                color=color, dmap=dmap, aux=aux)


def _share(got, want):
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / scale if scale > 0 else float(np.abs(got).max())


@functools.lru_cache(maxsize=None)
def _cut_grads(case, cut, dtype):
    f = frame(case)
    return S.full_reference_step(case, f["structure"], cut=cut, dtype=dtype, drop=f["drop"])[0]


# ---- 1. the forward is the oracles' -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FULL_CASES))
def test_restated_forward_is_the_oracles(case):
    import features_ref
    from helpers import image_report
    from oracle import backward_np as B
    from test_depth_cpu import depth_values_f32
    f, c = frame(case), FULL_CASES[case]
    st, keep, s, aux = f["st"], ~f["drop"], f["structure"], f["aux"]
    worst, bad, _ = image_report(f["color"] * keep, st["out_color"] * keep)
    worst_t, bad_t, _ = image_report(aux["finalT"] * keep, st["finalT"] * keep)
    assert ((aux["last"] == st["nContrib"]) | f["drop"]).all()
    line = f"[step full] {case}: image worst {worst:.3e}, finalT worst {worst_t:.3e}"
    assert bad == 0 and bad_t == 0, (case, worst, worst_t)
    cut = 1e-4 if c["profile"] == "inria" else 0.001
    if c["depth"]:
        d = depth_values_f32(f["scene"]["means3D"], np.asarray(f["cam"].view, np.float32), c["depth"] == "inverse").astype(np.float64)
        out64, _, _ = B.blend_forward(st["means2D"], st["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), s["ranges"], s["values"],
                                      W, H, (0.0, 0.0, 0.0), t_cutoff=cut)
        worst_d, bad_d, _ = image_report(f["dmap"] * keep, out64[0] * keep)
        line += f", depth worst {worst_d:.3e}"
        assert bad_d == 0, (case, worst_d)
    if c["channels"]:
        feat = features_ref.forward(st, f["raw"]["features"][:, :c["channels"]], None, W, H, t_cutoff=cut)
        assert (feat["nContrib"] == st["nContrib"]).all()
        worst_f, bad_f, _ = image_report(aux["feature_map"] * keep, feat["out"] * keep)
        line += f", features worst {worst_f:.3e}"
        assert bad_f == 0, (case, worst_f)
    if c["opacity"]:
        worst_a, bad_a, _ = image_report(aux["opacity_map"] * keep, (1.0 - st["finalT"].astype(np.float64)) * keep)
        line += f", opacity worst {worst_a:.3e}"
        assert bad_a == 0, (case, worst_a)
    print(line + f", {int(f['drop'].sum())} pixels dropped")
    # the smoothed nodes and c are the float32 restatements' (which the kernels are held to bit for bit elsewhere)
    vis = aux["visible"]
    if c["filter"]:
        sm = f["rows"]["smoothed"]
        assert _share(aux["scales_smoothed"].detach().numpy()[vis], sm["scales_out"][vis, :3].astype(np.float64)) <= 1e-6
        assert _share(aux["scales"].detach().numpy(), f["act"]["scales"][:, :3].astype(np.float64)) <= 1e-6
    if c["antialiased"]:
        assert np.abs(aux["compensation"].detach().numpy() - f["rows"]["masks"]["c"][vis]).max() <= 1e-5


# ---- 2. the float32 noise floor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FULL_CASES))
def test_float32_noise_floor_sets_the_gpu_bounds(case):
    f = frame(case)
    g32 = _cut_grads(case, None, R.F32)
    line = []
    for k in _arrays(case):
        want = f["grads"][k]
        if np.abs(want).max() == 0:
            assert (case, k) not in R.BOUNDS, (case, k)
            continue
        e32 = _share(g32[k], want)
        b = R.bound(case, k)
        line.append(f"{k} {e32:.1e}")
        assert b == R.FLOOR or 2 * e32 <= b <= 10 * e32, (case, k, e32, b)
        assert b >= 2 * e32, (case, k, e32, b)
    # ... and of dL_dmean2D, which the GPU test compares too
    e32 = _share(g32["per_gaussian.mean2D"], f["grads"]["per_gaussian.mean2D"])
    line.append(f"mean2D {e32:.1e}")
    assert R.bound(case, "mean2D") >= 2 * e32, (case, e32)
    print(f"[step full] {case}: e32: " + ", ".join(line))


# ---- 3. the cuts are seen ---------------------------------------------------------------------------------------------------
def cuts_of(case):
    """The new cuts that apply to a case -> the arrays of which at least one must move by more than 100 bounds."""
    c = FULL_CASES[case]
    out = {}
    if c["filter"]:
        out["filter_scale"] = ("log_scale",)
        out["filter_opacity"] = ("opacity_logit",)
        out["filter_coef"] = ("log_scale",)
    if c["antialiased"]:
        out["compensation"] = ("xyz", "log_scale", "rotation")
    if c["antialiased"] and c["filter"]:
        out["compensation_scales"] = ("log_scale",)
    if c["channels"]:
        out["feature_geometry"] = ("xyz", "opacity_logit", "log_scale", "rotation")
    if c["opacity"]:
        out["opacity_map"] = ("xyz", "opacity_logit", "log_scale", "rotation")
    return out


@pytest.mark.parametrize("case", list(FULL_CASES))
def test_every_new_cut_is_seen(case):
    f = frame(case)
    unseen = []
    for cut, arrays in cuts_of(case).items():
        g = _cut_grads(case, cut, R.F64)
        moved = {k: _share(g[k], f["grads"][k]) / R.bound(case, k) for k in arrays}
        print(f"[step full] {case}: cut {cut} moves " + ", ".join(f"{k} by {v:.0f} bounds" for k, v in moved.items()))
        if not max(moved.values()) > 100.0:
            unseen.append((cut, moved))
        assert all(np.isfinite(g[k]).all() for k in _arrays(case))
    assert not unseen, (case, unseen)


def test_the_modifier_before_the_smoothing_is_another_image():
    """scale_modifier multiplies the SMOOTHED scale (render smooths first; the rasterizer applies the modifier). The other
    order — the smoothing of the modified scale — moves the colour image of the case that has both by more than the image
    tolerance, so the image comparison of the GPU test tells the two apart."""
    case = "full-gscuda-m2"
    f = frame(case)
    cam = f["cam"]
    assert FULL_CASES[case]["scale_modifier"] != 1.0 and FULL_CASES[case]["filter"]
    color = R.forward(S.full_leaves(case), f["structure"], cam.tan_fovx, cam.tan_fovy, W, H,
                      **S.full_forward_options(case, modifier_first=True))[0].detach().numpy()
    moved = np.abs(color - f["color"]).max(0) * ~f["drop"]
    print(f"[step full] {case}: the modifier before the smoothing moves the image by {moved.max():.3e} ({int((moved > IMAGE_TOL).sum())} pixels)")
    assert moved.max() > 100 * IMAGE_TOL and (moved > IMAGE_TOL).sum() >= 0.1 * W * H


# ---- 4. conditions on the frames and the caps -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(FULL_CASES))
def test_frame_conditions(case):
    f, c = frame(case), FULL_CASES[case]
    s, aux = f["structure"], f["aux"]
    vis = s["vis"]
    third = vis.sum() / 3.0
    assert vis.sum() >= N / 2 and (~vis).sum() >= N / 8, (int(vis.sum()), N)
    if c["antialiased"]:
        comp = aux["compensation"].detach().numpy()
        print(f"[step full] {case}: c < 0.9 on {int((comp < 0.9).sum())}, > 0.9 on {int((comp > 0.9).sum())} of {vis.sum()} visible")
        assert (comp < 0.9).sum() >= third and (comp > 0.9).sum() >= third
        if c["profile"] == "inria":
            assert (vis & (s["clx"] | s["cly"]) & s["flows"]).any()
    if c["filter"]:
        coef = f["rows"]["smoothed"]["coef"][vis]
        ident = s["identity"][vis]
        print(f"[step full] {case}: filter coefficient < 0.9 on {int((~ident & (coef < 0.9)).sum())}, {int(ident.sum())} identity rows")
        assert (~ident & (coef < 0.9)).sum() >= third and ident.sum() >= 10
    if c["channels"]:
        # visible Gaussians that no pixel composites: their feature rows' gradients are exact zeros (asserted on the GPU)
        idle = int((~aux["blended"]).sum())
        print(f"[step full] {case}: {idle} visible Gaussians blend nothing")
        assert 0 < idle < vis.sum() / 2 and (f["grads"]["features"][aux["visible"][~aux["blended"]]] == 0).all()
    # the caps: at most 1 % of the pixels dropped, no Gaussian row left out
    assert f["drop"].sum() <= 0.01 * W * H, int(f["drop"].sum())
    near, differ = R.rows_near_a_threshold(aux, s, f["cam"].tan_fovx, f["cam"].tan_fovy,
                                           S.filter_values(case), c["antialiased"])
    assert not near.any() and not differ.any(), (case, np.nonzero(near)[0], np.nonzero(differ)[0])
    for k in _arrays(case)[:5]:
        if k == "shs" and not c["colour"]:
            assert (f["grads"][k] == 0).all()
            continue
        rows = np.abs(f["grads"][k].reshape(N, -1)).max(1) > 0
        assert rows.sum() >= N / 4, (k, int(rows.sum()))


def test_the_old_cases_do_not_see_the_new_options():
    """forward() with every new option at its default is the forward the seven CASES are pinned with: no new key of the
    structure is read, and the result carries no map."""
    import test_step_autograd_cpu as old
    f = old.frame("inria-3-depth")
    assert not {"flows", "floored", "d1_bad", "identity"} & set(f["structure"])
    assert f["aux"]["feature_map"] is None and f["aux"]["opacity_map"] is None and f["aux"]["compensation"] is None
