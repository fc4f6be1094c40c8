"""CPU: the float64 autograd reference of the training step (tests/step_autograd_ref.py) — its forward pinned to the CPU
oracles' images, its gradient compared with the hand-derived oracle's, the float32 noise floor that sets the GPU test's
bounds, the cuts (blindness guards) and the conditions on the frames. No GPU, no library kernel: the frames are those of
tests/test_gpu_step_autograd.py (tests/step_frames.py), their structure the CPU oracles'.

Measured figures (this file prints them; `pytest -s`), as shares of an array's largest entry (images: absolute, per pixel).

1. The forward (no frame drops a pixel):
  case                 image    finalT   depth
  gscuda               4.8e-7   6.6e-7   -
  gscuda-depth         4.8e-7   6.6e-7   2.6e-6
  gscuda-inverse-m2    3.7e-7   2.3e-7   7.3e-8
  inria-3-depth        3.2e-7   2.2e-7   9.2e-7
  inria-0-m0.5         4.4e-7   9.9e-7   -
  inria-2-inverse-kx   3.5e-7   1.8e-7   4.3e-8
  inria-precomp        2.4e-7   2.2e-7   -

2. Autograd against the whole hand-derived composition started from the oracle's FLOAT32 forward state (and the float32
activated arrays); AGREEMENT asserts ten times each figure:
  case               means3D scales  rotat.s opacit. xyz     op_logit log_sc. rotation shs|col view    proj    cam_pos
  gscuda             6.7e-7  2.6e-7  1.7e-6  1.6e-7  6.7e-7  6.0e-7  2.6e-7  1.2e-6  2.7e-7  2.3e-7  4.2e-7  0
  gscuda-depth       4.4e-7  3.1e-7  1.4e-6  3.9e-7  4.4e-7  3.9e-7  3.1e-7  9.6e-7  2.7e-7  1.1e-7  2.2e-7  0
  gscuda-inverse-m2  1.1e-7  5.5e-7  9.0e-7  3.3e-7  1.1e-7  8.2e-7  5.5e-7  9.1e-7  2.8e-7  1.5e-7  8.7e-7  0
  inria-3-depth      1.5e-7  5.0e-7  4.3e-7  8.5e-8  1.5e-7  8.4e-8  3.5e-7  6.4e-7  1.2e-7  9.6e-8  4.1e-7  4.3e-8
  inria-0-m0.5       2.3e-6  1.0e-6  3.6e-7  2.6e-7  2.3e-6  2.8e-7  5.0e-7  2.6e-6  2.4e-7  5.7e-7  3.1e-6  0
  inria-2-inverse-kx 1.5e-7  2.3e-7  1.2e-7  6.9e-8  1.5e-7  6.9e-8  2.3e-7  2.1e-6  5.8e-8  7.7e-8  1.6e-7  3.0e-7
  inria-precomp      2.0e-7  1.6e-7  2.8e-7  1.8e-7  2.0e-7  1.5e-7  1.6e-7  1.1e-6  1.1e-7  3.8e-7  3.3e-7  0
Ten times the figure is at least ten times tighter than the GPU's 2e-4 for every array but four: xyz (= means3D) 2.4e-5,
rotation 2.6e-5 and proj 3.1e-5 of inria-0-m0.5, and rotation 2.1e-5 of inria-2-inverse-kx (FLOAT32_STATE_PAIRS). Neither
reference is wrong there. Fed the restatement's own float64 state, every hand-derived piece returns autograd's gradient
(3. below), so what is left is the float32 state, amplified where an array is a small difference of large terms: the raw
quaternion's gradient is the activated one's projected off the quaternion (under the upstream profile most of it lies along
it), proj's is a sum over the Gaussians that cancels, and with modifier 0.5 the 0.3 dilation dominates cov2D. For these four
the test asserts what that account implies: the figure stays within FLOAT32_STATE_FACTOR times the same array's e32 on the
same frame (measured 1.9, 0.7, 2.0 and 0.6 times).

3. Every hand-derived piece on the restatement's float64 state, worst over the cases (PIECE_TOL asserts ten times each; the
chain's rest is the helpers' float64 focal length against the library's float32 one, the camera view block's the float32
t.z of camera_grad_ref's decisions; 1e-12 where only double rounding is left):
  blend: mean2D 1.2e-9, cov2D 6.4e-10, colors 3.7e-9, opacities 1.5e-9, depths 1.7e-10
  chain: means3D 2.1e-8, scales 2.6e-8, rotations 4.7e-8, shs 6e-18
  camera: view 2.2e-7, proj 1e-15, cam_pos 1e-15;  activation: xyz 0, opacity_logit 4e-16, log_scale 0, rotation 8e-15

4. e32, the float32 restatement against the float64 one:
  case               xyz     op_logit log_sc. rotation shs|col view    proj    cam_pos
  gscuda             6.3e-7  6.8e-7  5.3e-7  1.3e-6  3.8e-7  7.2e-7  7.3e-7  -
  gscuda-depth       4.1e-7  4.4e-7  3.2e-7  9.2e-7  3.8e-7  4.4e-7  3.0e-7  -
  gscuda-inverse-m2  8.4e-8  7.6e-7  6.1e-7  9.8e-7  6.8e-7  1.8e-7  3.5e-7  -
  inria-3-depth      3.3e-7  1.4e-7  3.4e-7  1.6e-6  7.0e-7  3.4e-7  1.5e-6  3.3e-7
  inria-0-m0.5       1.2e-6  2.7e-7  3.6e-7  3.5e-6  3.2e-7  1.8e-7  1.6e-6  -
  inria-2-inverse-kx 3.1e-7  2.0e-7  3.0e-7  3.5e-6  3.3e-7  1.9e-7  4.1e-7  7.9e-7
  inria-precomp      1.9e-7  2.2e-7  5.3e-7  3.0e-6  4.6e-7  6.6e-7  2.6e-7  -
2 e32 stays below 2e-4 everywhere: every GPU bound is 2e-4 (on the GPU the worst array sits at 2.7e-6,
tests/test_gpu_step_autograd.py).
"""
import functools

import numpy as np
import pytest

import activation_ref as A
import step_autograd_ref as R
import step_frames as S
from camera_grad_ref import camera_grad
from step_frames import BG, CASES, H, N, W

ACTIVATED = ("means3D", "scales", "rotations", "opacities")
# The bound of the comparison with the whole hand-derived composition, per case and array, as a share of the array's largest
# entry: ten times the measured disagreement (docstring, 2.), rounded up to two digits. The two float64 gradients differ in
# that oracle/backward_np.py starts from the float32 forward state. 0.0: both are identically zero.
AGREEMENT = {
    "gscuda": {"means3D": 6.8e-6, "scales": 2.7e-6, "rotations": 1.7e-5, "opacities": 1.6e-6, "xyz": 6.8e-6, "opacity_logit": 6.0e-6,
               "log_scale": 2.7e-6, "rotation": 1.3e-5, "shs": 2.7e-6, "view": 2.4e-6, "proj": 4.3e-6, "cam_pos": 0.0},
    "gscuda-depth": {"means3D": 4.4e-6, "scales": 3.1e-6, "rotations": 1.5e-5, "opacities": 3.9e-6, "xyz": 4.4e-6,
                     "opacity_logit": 4.0e-6, "log_scale": 3.1e-6, "rotation": 9.7e-6, "shs": 2.7e-6, "view": 1.2e-6, "proj": 2.3e-6,
                     "cam_pos": 0.0},
    "gscuda-inverse-m2": {"means3D": 1.2e-6, "scales": 5.5e-6, "rotations": 9.1e-6, "opacities": 3.4e-6, "xyz": 1.2e-6,
                          "opacity_logit": 8.3e-6, "log_scale": 5.5e-6, "rotation": 9.1e-6, "shs": 2.9e-6, "view": 1.5e-6,
                          "proj": 8.8e-6, "cam_pos": 0.0},
    "inria-3-depth": {"means3D": 1.6e-6, "scales": 5.0e-6, "rotations": 4.3e-6, "opacities": 8.5e-7, "xyz": 1.6e-6,
                      "opacity_logit": 8.5e-7, "log_scale": 3.5e-6, "rotation": 6.4e-6, "shs": 1.2e-6, "view": 9.6e-7, "proj": 4.1e-6,
                      "cam_pos": 4.4e-7},
    "inria-0-m0.5": {"means3D": 2.4e-5, "scales": 1.1e-5, "rotations": 3.7e-6, "opacities": 2.7e-6, "xyz": 2.4e-5,
                     "opacity_logit": 2.8e-6, "log_scale": 5.0e-6, "rotation": 2.6e-5, "shs": 2.4e-6, "view": 5.8e-6, "proj": 3.1e-5,
                     "cam_pos": 0.0},
    "inria-2-inverse-kx": {"means3D": 1.6e-6, "scales": 2.4e-6, "rotations": 1.2e-6, "opacities": 7.0e-7, "xyz": 1.6e-6,
                           "opacity_logit": 7.0e-7, "log_scale": 2.4e-6, "rotation": 2.1e-5, "shs": 5.8e-7, "view": 7.8e-7,
                           "proj": 1.6e-6, "cam_pos": 3.1e-6},
    "inria-precomp": {"means3D": 2.0e-6, "scales": 1.6e-6, "rotations": 2.9e-6, "opacities": 1.8e-6, "xyz": 2.0e-6,
                      "opacity_logit": 1.5e-6, "log_scale": 1.6e-6, "rotation": 1.1e-5, "colors": 1.2e-6, "view": 3.8e-6,
                      "proj": 3.4e-6, "cam_pos": 0.0},
}
# The (case, array) pairs whose AGREEMENT is not ten times tighter than the GPU's bound (docstring, 2.: the float32 state,
# not a wrong reference). What that account implies is asserted instead: the disagreement is float32 rounding of the forward
# state, of which e32 — float32 rounding of the same quantities in the restatement — is another realisation on the same frame
# and array, so the two worst entries lie within a small factor of each other. 4 = 2 for the spread between the maxima of two
# realisations of the same noise, times 2 because the hand-derived path also reads float32 activated arrays that the float32
# restatement recomputes.
FLOAT32_STATE_PAIRS = (("inria-0-m0.5", "means3D"), ("inria-0-m0.5", "xyz"), ("inria-0-m0.5", "rotation"), ("inria-0-m0.5", "proj"),
                       ("inria-2-inverse-kx", "rotation"))
FLOAT32_STATE_FACTOR = 4.0
# piece by piece on the float64 state: ten times the worst measured over the cases (docstring, 3.)
PIECE_TOL = {"blend: mean2D": 1.2e-8, "blend: cov2D": 6.4e-9, "blend: colors": 3.7e-8, "blend: opacities": 1.5e-8,
             "blend: depths": 1.7e-9, "chain: means3D": 2.1e-7, "chain: scales": 2.6e-7, "chain: rotations": 4.7e-7,
             "chain: shs": 1e-12, "camera: view": 2.2e-6, "camera: proj": 1e-12, "camera: cam_pos": 1e-12,
             "activation: xyz": 1e-12, "activation: opacity_logit": 1e-12, "activation: log_scale": 1e-12,
             "activation: rotation": 1e-12}

def _arrays(case):
    """The gradient arrays of a case: the raw parameters (the colours instead of shs through colors_precomp) and the camera."""
    precomp = CASES[case][5]
    return ("xyz", "opacity_logit", "log_scale", "rotation", "colors" if precomp else "shs", "view", "proj", "cam_pos")


@functools.lru_cache(maxsize=None)
def frame(case):
    """The case's frame on the CPU: scene, camera, the oracle's forward state, the structure, and the float64 reference step
    (gradients, image, depth, dropped pixels)."""
    from oracle import cpu_oracle, inria_np
    profile, deg, depth, mod, kx, precomp = CASES[case]
    raw = S.raw_scene(profile)
    cam = S.camera_of(case)
    scene = S.activated_scene(raw)
    colors = raw["colors"] if precomp else None
    if profile == "inria":
        st = inria_np.forward(scene, cam, BG, deg=deg, scale_modifier=mod, blend_with="numpy-expf", colors_precomp=colors)
    else:
        st = cpu_oracle.forward(scene, cam, BG, scale_modifier=mod)
    structure = S.structure_of(raw, cam, st["radii"], st["ranges"], st["values"], st["nContrib"], st.get("clamped"))
    w, wd = S.weights()
    grads, color, dmap, aux, drop = S.reference_step(raw, cam, case, structure, w, wd)
    return dict(case=case, raw=raw, cam=cam, scene=scene, st=st, structure=structure, w=w, wd=wd, drop=drop, grads=grads,
                color=color, dmap=dmap, aux=aux, colors=colors)


def _share(got, want):
    """The largest difference of two arrays as a share of the reference's largest entry."""
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / scale if scale > 0 else float(np.abs(got).max())


@functools.lru_cache(maxsize=None)
def _cut_grads(case, cut, dtype):
    f = frame(case)
    return S.reference_step(f["raw"], f["cam"], case, f["structure"], f["w"], f["wd"], cut=cut, dtype=dtype, drop=f["drop"])[0]


# ---- 1. the forward is the oracle's ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_restated_forward_is_the_oracles(case):
    from helpers import image_report
    from oracle import backward_np as B
    from test_depth_cpu import depth_values_f32
    f = frame(case)
    st, keep = f["st"], ~f["drop"]
    worst, bad, _ = image_report(f["color"] * keep, st["out_color"] * keep)
    worst_t, bad_t, _ = image_report(f["aux"]["finalT"] * keep, st["finalT"] * keep)
    print(f"[step autograd] {case}: image worst {worst:.3e}, finalT worst {worst_t:.3e}, {int(f['drop'].sum())} pixels dropped")
    assert bad == 0 and bad_t == 0, (case, worst, worst_t)
    depth = CASES[case][2]
    if depth:
        d = depth_values_f32(f["scene"]["means3D"], np.asarray(f["cam"].view, np.float32), depth == "inverse").astype(np.float64)
        s = f["structure"]
        cut = 1e-4 if CASES[case][0] == "inria" else 0.001
        out64, _, _ = B.blend_forward(st["means2D"], st["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), s["ranges"], s["values"],
                                      W, H, (0.0, 0.0, 0.0), t_cutoff=cut)
        worst_d, bad_d, _ = image_report(f["dmap"] * keep, out64[0] * keep)
        print(f"[step autograd] {case}: depth worst {worst_d:.3e}")
        assert bad_d == 0, (case, worst_d)


# ---- 2. autograd against the hand-derived oracle ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hand_derived(case):
    """The same step's gradients from oracle/backward_np.py over the oracle's float32 forward state, composed as the GPU tests
    compose them: blend backward (+ the depth channel's superposition) -> helpers.backward_chain_expected[_inria] (+ the depth
    term of the mean) -> activation_ref.backward; the camera from camera_grad_ref.camera_grad."""
    from helpers import backward_chain_expected, backward_chain_expected_inria
    from oracle import backward_np as B
    from test_depth_cpu import depth_mean_term, depth_values_f32
    f = frame(case)
    profile, deg, depth, mod, kx, precomp = CASES[case]
    inria = profile == "inria"
    st, s, cam, scene, raw = f["st"], f["structure"], f["cam"], f["scene"], f["raw"]
    keep = ~f["drop"]
    rgb = f["colors"] if precomp else st["rgb"]
    cut = 1e-4 if inria else 0.001
    _, ft64, nc64 = B.blend_forward(st["means2D"], st["conicOpacity"], rgb, s["ranges"], s["values"], W, H, BG, t_cutoff=cut)
    e = B.blend_backward(st["means2D"], st["conicOpacity"], rgb, s["ranges"], s["values"], nc64, ft64, W, H, BG, f["w"] * keep)
    d_mean, d_conic, d_op, dd = e["dL_dmean2D"], e["dL_dconic"], e["dL_dopacity"].reshape(N), None
    if depth:
        d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), depth == "inverse").astype(np.float64)
        g3 = np.zeros((3, H, W))
        g3[0] = f["wd"] * keep
        ed = B.blend_backward(st["means2D"], st["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), s["ranges"], s["values"], nc64, ft64,
                              W, H, (0.0, 0.0, 0.0), g3)
        d_mean, d_conic, d_op = d_mean + ed["dL_dmean2D"], d_conic + ed["dL_dconic"], d_op + ed["dL_dopacity"].reshape(N)
        dd = ed["dL_dcolor"][:, 0]
    co = st["conicOpacity"].astype(np.float64)
    K = np.stack([np.stack([co[:, 0], co[:, 1]], 1), np.stack([co[:, 1], co[:, 2]], 1)], 1)
    gK = np.stack([np.stack([d_conic[:, 0], 0.5 * d_conic[:, 1]], 1), np.stack([0.5 * d_conic[:, 1], d_conic[:, 2]], 1)], 1)
    gM = -K @ gK @ K
    d_cov = np.stack([gM[:, 0, 0], gM[:, 0, 1], gM[:, 1, 1]], 1)
    up = {"dL_dmean2D": d_mean, "dL_dconic_opacity": np.concatenate([d_conic, d_op[:, None]], 1), "dL_dcov2D": d_cov,
          "dL_dcolors": e["dL_dcolor"]}
    vis = np.nonzero(s["vis"])[0]
    g_state = {"cov3D": st["cov3D"], "rgb": st["rgb"]}
    if inria:
        sc = dict(scene, shs=scene["shs"] if not precomp else np.zeros_like(scene["shs"]))
        ch = backward_chain_expected_inria(None, g_state, sc, cam, W, H, vis, deg, s["clamped"], upstream=up, scale_modifier=mod)
    else:
        ch = backward_chain_expected(None, g_state, scene, cam, W, H, vis, upstream=up, scale_modifier=mod)
    full = {k: np.zeros((N, 4)) for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations")}
    full["dL_dmeans3D"][vis, :3] = ch["dL_dmeans3D"]
    if depth:
        full["dL_dmeans3D"][vis, :3] += depth_mean_term(scene["means3D"][:, :3], np.asarray(cam.view, np.float32), dd, depth == "inverse")[vis]
    full["dL_dscales"][vis, :3] = ch["dL_dscales"]
    full["dL_drotations"][vis] = ch["dL_drotations"]
    out = {"means3D": full["dL_dmeans3D"][:, :3], "scales": full["dL_dscales"][:, :3], "rotations": full["dL_drotations"],
           "opacities": d_op}
    if precomp:
        out["colors"] = e["dL_dcolor"]
    elif inria:
        out["shs"] = np.zeros((N, 48))
        out["shs"][vis] = ch["dL_dshs"]
    else:
        out["shs"] = np.zeros((N, 48))
        out["shs"][:, :3] = 0.4 * e["dL_dcolor"]
    g, _ = camera_grad(scene["means3D"], cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, W, H, st["radii"],
                       g_state["cov3D"], d_mean, d_cov, dL_ddepths=dd, inverse=depth == "inverse", inria=inria,
                       shs=scene["shs"] if inria and not precomp else None, sh_degree=deg, dL_dcolors=e["dL_dcolor"] if inria else None,
                       clamped=s["clamped"] if inria else None)
    out["view"], out["proj"], out["cam_pos"] = g[:16], g[16:32], g[32:]
    d_xyz, d_o, d_s, d_r = A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], full["dL_dmeans3D"], full["dL_dscales"],
                                      full["dL_drotations"], d_op, radii=st["radii"])
    out.update(xyz=d_xyz, opacity_logit=d_o, log_scale=d_s, rotation=d_r)
    return out


def _full(rows, vis):
    """Rows of the visible Gaussians scattered into an array over all N (zeros elsewhere)."""
    out = np.zeros((N,) + rows.shape[1:])
    out[vis] = rows
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_each_hand_derived_piece_agrees_with_autograd_in_float64(case):
    """The same comparison piece by piece, with the float32 forward state taken out: every hand-derived piece is fed the
    restatement's own float64 per-Gaussian state and autograd's own gradient of that piece's output, and must return
    autograd's gradient of its input — the blend backward, the chain with its depth term, the camera reference, the
    activations. What is left between the two is float64 rounding (and the chain's focal length, which the helpers form in
    float64 and the library and the restatement in float32: 6e-8)."""
    from helpers import backward_chain_expected, backward_chain_expected_inria
    from oracle import backward_np as B
    from test_depth_cpu import depth_mean_term
    f = frame(case)
    profile, deg, depth, mod, kx, precomp = CASES[case]
    inria = profile == "inria"
    g, aux, cam, s, raw = f["grads"], f["aux"], f["cam"], f["structure"], f["raw"]
    vis = aux["visible"]
    keep = ~f["drop"]
    val = lambda k: aux["per_gaussian"][k].detach().numpy()
    cov = val("cov2D")
    det = cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2
    conic_o = _full(np.stack([cov[:, 2] / det, -cov[:, 1] / det, cov[:, 0] / det, aux["opacities"].detach().numpy()[vis]], 1), vis)
    m2, rgb = _full(val("mean2D"), vis), _full(val("colors"), vis)
    gc = g["per_gaussian.cov2D"]
    auto = {"dL_dmean2D": _full(g["per_gaussian.mean2D"], vis), "dL_dcolors": _full(g["per_gaussian.colors"], vis),
            # (cov2D's b stands for both off-diagonal entries: the gradient of the symmetric matrix's entry is half of b's)
            "dL_dcov2D": _full(np.stack([gc[:, 0], 0.5 * gc[:, 1], gc[:, 2]], 1), vis), "dL_dconic_opacity": np.zeros((N, 4))}
    dd = _full(g["per_gaussian.depths"], vis) if depth else None
    worst = {}
    # -- the blend backward
    cut = 1e-4 if inria else 0.001
    _, ft64, nc64 = B.blend_forward(m2, conic_o, rgb, s["ranges"], s["values"], W, H, BG, t_cutoff=cut)
    assert ((nc64 == aux["last"]) | f["drop"]).all()
    e = B.blend_backward(m2, conic_o, rgb, s["ranges"], s["values"], nc64, ft64, W, H, BG, f["w"] * keep)
    d_mean, d_conic, d_op, d_col = e["dL_dmean2D"], e["dL_dconic"], e["dL_dopacity"].reshape(N), e["dL_dcolor"]
    if depth:
        d = _full(val("depths"), vis)
        g3 = np.zeros((3, H, W))
        g3[0] = f["wd"] * keep
        ed = B.blend_backward(m2, conic_o, np.stack([d, 0 * d, 0 * d], 1), s["ranges"], s["values"], nc64, ft64, W, H, (0.0, 0.0, 0.0), g3)
        d_mean, d_conic, d_op = d_mean + ed["dL_dmean2D"], d_conic + ed["dL_dconic"], d_op + ed["dL_dopacity"].reshape(N)
        worst["blend: depths"] = _share(ed["dL_dcolor"][:, 0], dd)
    K = np.stack([np.stack([conic_o[:, 0], conic_o[:, 1]], 1), np.stack([conic_o[:, 1], conic_o[:, 2]], 1)], 1)
    gK = np.stack([np.stack([d_conic[:, 0], 0.5 * d_conic[:, 1]], 1), np.stack([0.5 * d_conic[:, 1], d_conic[:, 2]], 1)], 1)
    gM = -K @ gK @ K
    worst["blend: mean2D"] = _share(d_mean, auto["dL_dmean2D"])
    worst["blend: cov2D"] = _share(np.stack([gM[:, 0, 0], gM[:, 0, 1], gM[:, 1, 1]], 1), auto["dL_dcov2D"])
    worst["blend: colors"] = _share(d_col, auto["dL_dcolors"])
    worst["blend: opacities"] = _share(d_op, g["opacities"])
    # -- the chain
    act = lambda k, pad: np.concatenate([aux[k].detach().numpy(), np.full((N, 1), pad)], 1)
    scene64 = {"means3D": act("means3D", 1.0), "scales": act("scales", np.e), "rotations": aux["rotations"].detach().numpy(),
               "shs": raw["shs"].astype(np.float64) if not precomp else np.zeros((N, 48))}
    state = {"cov3D": _full(aux["cov3D"].numpy(), vis), "rgb": rgb}
    if inria:
        ch = backward_chain_expected_inria(None, state, scene64, cam, W, H, vis, deg, s["clamped"], upstream=auto, scale_modifier=mod)
    else:
        ch = backward_chain_expected(None, state, scene64, cam, W, H, vis, upstream=auto, scale_modifier=mod)
    mean = ch["dL_dmeans3D"]
    if depth:
        mean = mean + depth_mean_term(scene64["means3D"][:, :3], np.asarray(cam.view, np.float32), dd, depth == "inverse")[vis]
    worst["chain: means3D"] = _share(mean, g["means3D"][vis])
    worst["chain: scales"] = _share(ch["dL_dscales"], g["scales"][vis])
    worst["chain: rotations"] = _share(ch["dL_drotations"], g["rotations"][vis])
    if inria and not precomp:
        worst["chain: shs"] = _share(ch["dL_dshs"], g["shs"][vis])
    # -- the camera
    radii = s["vis"].astype(np.int32)
    cg, _ = camera_grad(scene64["means3D"], cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, W, H, radii, state["cov3D"],
                        auto["dL_dmean2D"], auto["dL_dcov2D"], dL_ddepths=dd, inverse=depth == "inverse", inria=inria,
                        shs=raw["shs"] if inria and not precomp else None, sh_degree=deg, dL_dcolors=auto["dL_dcolors"] if inria else None,
                        clamped=s["clamped"] if inria else None)
    worst["camera: view"], worst["camera: proj"] = _share(cg[:16], g["view"]), _share(cg[16:32], g["proj"])
    worst["camera: cam_pos"] = _share(cg[32:], g["cam_pos"])
    # -- the activations
    pad = lambda a: np.concatenate([a, np.zeros((N, 1))], 1)
    back = A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], pad(g["means3D"]), pad(g["scales"]), g["rotations"], g["opacities"])
    for k, a in zip(("xyz", "opacity_logit", "log_scale", "rotation"), back):
        worst["activation: " + k] = _share(a, g[k])
    print(f"[step autograd] {case}: pieces in float64: " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= PIECE_TOL[k], (case, k, v)


@pytest.mark.parametrize("case", list(CASES))
def test_autograd_agrees_with_the_hand_derived_oracle(case):
    f = frame(case)
    hand = hand_derived(case)
    g32 = _cut_grads(case, None, R.F32)
    for k in ACTIVATED + _arrays(case):
        got, want = f["grads"][k], hand[k]
        share = _share(got.reshape(want.shape), want)
        print(f"[step autograd] {case}: {k} autograd vs hand-derived {share:.3e} of the largest entry")
        assert share <= AGREEMENT[case][k], (case, k, share)
        # ... at least ten times tighter than the GPU's bound for the array, or one of the two references is wrong
        raw_k = {"means3D": "xyz", "scales": "log_scale", "rotations": "rotation", "opacities": "opacity_logit"}.get(k, k)
        if (case, k) in FLOAT32_STATE_PAIRS:
            e32 = _share(g32[raw_k], f["grads"][raw_k])              # (means3D is xyz: the activation is the identity)
            print(f"[step autograd] {case}: {k} disagreement is {share / e32:.2f} of the array's e32")
            assert share <= FLOAT32_STATE_FACTOR * e32, (case, k, share, e32)
        else:
            assert AGREEMENT[case][k] <= 0.1 * R.bound(case, raw_k), (case, k)


# ---- 3. the float32 noise floor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_float32_noise_floor_sets_the_gpu_bounds(case):
    f = frame(case)
    g32 = _cut_grads(case, None, R.F32)
    for k in _arrays(case):
        want = f["grads"][k]
        if want is None or np.abs(want).max() == 0:
            assert (case, k) not in R.BOUNDS, (case, k)
            continue
        e32 = _share(g32[k], want)
        b = R.bound(case, k)
        print(f"[step autograd] {case}: e32[{k}] = {e32:.3e}, bound {b:.1e}")
        assert b == 2e-4 or 2 * e32 <= b <= 10 * e32, (case, k, e32, b)
        assert b >= 2 * e32, (case, k, e32, b)


# ---- 4. the cuts are seen ---------------------------------------------------------------------------------------------------
BG_ARRAYS = ("xyz", "opacity_logit", "log_scale", "rotation")


def cuts_of(case):
    """The cuts that apply to a case -> the per-Gaussian arrays and the camera blocks each must show in (the background
    reaches every array through the final T; the quaternion norm, the modifier and W's dependence on the view matrix reach
    one array each and nothing else). view_direction needs SH beyond the DC term, depth_mean a depth channel, modifier a
    modifier other than 1. clamp_to_tz needs visible Gaussians beyond +-1.3 tan(fov): the upstream profile shows the
    scene's eight; the gscuda profile culls by the NDC position first and meets a clamped one only in a window of 1e-3 of
    the limit (tests/test_gpu_backward_poses.py, _clamp_scene), which stays that test's business."""
    profile, deg, depth, mod, kx, precomp = CASES[case]
    inria = profile == "inria"
    out = {"background": (BG_ARRAYS, ("view", "proj")),
           "jacobian_mean": (("xyz",), ("view",)),
           "quat_norm": (("rotation",), ()),
           "cov2D_view": ((), ("view",))}
    if inria and deg > 0 and not precomp:
        out["view_direction"] = (("xyz",), ("cam_pos",))
    if depth:
        out["depth_mean"] = (("xyz",), ("view",))
    if inria:
        out["clamp_to_tz"] = (("xyz",), ("view",))
    if mod != 1.0:
        out["modifier"] = (("log_scale",), ())
    return out


def _rows_seen(true, cut, tol):
    from helpers import _rows_differ
    return _rows_differ(true.reshape(true.shape[0], -1), cut.reshape(true.shape[0], -1), 10 * tol)


@pytest.mark.parametrize("case", list(CASES))
def test_every_cut_is_seen(case):
    """The reference with one coupling detached differs from the true one by more than ten times the case's bound: per
    Gaussian on its own largest component on at least a quarter of the Gaussians the coupling reaches (the visible ones;
    for the clamp's path to t.z the visible clamped ones), and for the camera on at least one entry of the affected block."""
    from test_gpu_backward_poses import _guard_share
    f = frame(case)
    s = f["structure"]
    vis = s["vis"]
    for cut, (arrays, blocks) in cuts_of(case).items():
        g = _cut_grads(case, cut, R.F64)
        rows = vis & (s["clx"] | s["cly"]) if cut == "clamp_to_tz" else vis
        assert rows.sum() >= 4, (case, cut, int(rows.sum()))
        for k in arrays:
            seen = _rows_seen(f["grads"][k][rows], g[k][rows], R.bound(case, k))
            print(f"[step autograd] {case}: cut {cut} seen in {k} on {int(seen.sum())} of {seen.size} Gaussians")
            _guard_share(seen, f"{case}: cut {cut} in {k}")
        for block in blocks:
            true = f["grads"][block]
            diff = np.abs(g[block] - true)
            print(f"[step autograd] {case}: cut {cut} moves {block} by {float(diff.max() / np.abs(true).max()):.3e} of its largest entry")
            assert (diff > 10 * R.bound(case, block) * np.abs(true).max()).any(), (case, cut, block)


# ---- 5. conditions on the frames --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_frame_conditions(case):
    from oracle import backward_np as B
    f = frame(case)
    profile, deg, depth, mod, kx, precomp = CASES[case]
    st, s = f["st"], f["structure"]
    vis = s["vis"]
    assert vis.sum() >= N / 2 and (~vis).sum() >= N / 8, (int(vis.sum()), N)
    # from the oracle's state, pixel by pixel over its tile's list: a record composited with alpha clamped at 0.99 (by
    # 1e-3 at least), and a pixel that stops at the cut-off — behind its last contributor comes a record that passes the
    # 1/255 test and would take the oracle's finalT below the cut-off
    cut = 1e-4 if profile == "inria" else 0.001
    gx = (W + 15) // 16
    o = st["conicOpacity"].astype(np.float64)
    m2 = st["means2D"].astype(np.float64)
    clamped99 = stopped = 0
    for y, x in zip(*np.nonzero(st["nContrib"] > 0)):
        t = (y // 16) * gx + x // 16
        ids = s["values"][s["ranges"][t, 0]:s["ranges"][t, 1]]
        dx, dy = m2[ids, 0] - x, m2[ids, 1] - y
        power = -0.5 * (o[ids, 0] * dx * dx + o[ids, 2] * dy * dy) - o[ids, 1] * dx * dy
        a_raw = o[ids, 3] * np.exp(power)
        live = (power <= 0) & (a_raw >= 1.0 / 255.0)
        nc = int(st["nContrib"][y, x])
        clamped99 += int((live[:nc] & (a_raw[:nc] > 0.99 * (1 + 1e-3))).any())
        after = np.nonzero(live[nc:])[0]
        if after.size:
            stopped += int(float(st["finalT"][y, x]) * (1.0 - min(0.99, a_raw[nc + after[0]])) < cut)
    print(f"[step autograd] {case}: {stopped} pixels stop at the cut-off, {clamped99} composite a record clamped at 0.99")
    assert clamped99 > 0 and stopped > 0
    if profile == "inria" and not precomp:
        assert s["clamped"][vis].any()
    if profile == "inria":
        assert (vis & (s["clx"] | s["cly"])).sum() >= 4
    for k in _arrays(case)[:5]:
        rows = np.abs(f["grads"][k].reshape(N, -1)).max(1) > 0
        assert rows.sum() >= N / 4, (k, int(rows.sum()))
    assert f["drop"].sum() <= 0.01 * W * H, int(f["drop"].sum())
    assert f["drop"].sum() < (~f["drop"]).sum()
