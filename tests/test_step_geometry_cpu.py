"""CPU: the float64 autograd reference of the training step (tests/step_autograd_ref.py) with the three geometry regularisers
autograd.render composes around the rasterizer — the distortion map, the normal map with the normal-consistency term, the median
map — on the frames of tests/test_gpu_step_geometry.py (tests/step_frames.py, GEOMETRY_CASES). As tests/test_step_full_cpu.py
does for the filter, the compensation and the feature map: the forward pinned to the CPU references of each map and the
gradient to central differences, the float32 noise floor that sets the GPU test's bounds, the cuts (blindness guards), the
conditions on the frames and the caps. No GPU, no library kernel: the structure is the CPU oracles', the median ids
median_ref.forward's, the decisions of the normals normals_ref's float32 restatements on the oracle's float32 maps.

Measured figures (this file prints them; `pytest -s`), as shares of an array's largest entry (images: absolute, per pixel).

1. The forward's maps against the float32 references (distortion_ref.forward32, median_ref.forward, features_ref's replay of
gaussian_normals_f32 and of the view depth, the oracles' image and finalT); no frame drops a pixel, erosion and the depth
normals' decisions take none from the consistency term, no Gaussian row is near a threshold; the median ids are equal everywhere:
  case                   image   finalT  depth   distortion median  normals features
  2dgs-inria             2.2e-7  3.1e-7  6.2e-7  5.7e-7     -       1.5e-7  -
  2dgs-gscuda-median     1.0e-6  1.2e-6  5.3e-6  6.4e-7     5.3e-7  1.2e-6  -
  pose-distortion-median 5.4e-7  7.8e-7  2.9e-6  2.0e-6     4.3e-7  -       -
  value-tensors          1.0e-6  1.2e-6  -       1.8e-6     0       1.2e-6  2.1e-6
  normals-alone          3.9e-7  5.8e-7  -       -          -       4.4e-7  -
The autograd gradient against central differences of the reference's own float64 loss (step 1e-6; the two largest entries of
xyz, rotation and, where it is a leaf, view): they differ by at most 7e-8, on entries of 0.8 .. 160, on 2dgs-inria and
pose-distortion-median. The
differences hold opacity.detach() at the frame's value: it is a constant of the function that is differentiated.

2. e32, the float32 restatement against the float64 one, on the same structure, dropped pixels and keep_n:
  case                   xyz     op_logit log_sc. rotation shs     features values(d, m)   view    proj    cam_pos mean2D
  2dgs-inria             2.3e-6  3.7e-7  1.4e-6  7.1e-7  9.1e-7  -        -              const   3.2e-6  4.0e-7  2.3e-6
  2dgs-gscuda-median     1.0e-6  7.5e-7  1.1e-6  3.3e-6  6.2e-7  -        -              const   1.4e-6  -       2.1e-6
  pose-distortion-median 2.4e-6  2.8e-7  1.0e-7  6.0e-7  1.3e-6  -        -              1.7e-7  2.7e-7  1.7e-6  1.2e-6
  value-tensors          8.4e-7  8.4e-7  9.4e-7  1.4e-6  0       1.1e-6   4.8e-7, 9.7e-8 const   8.9e-7  -       7.3e-7
  normals-alone          1.4e-6  5.5e-7  1.9e-6  9.6e-7  0       -        -              const   2.3e-7  -       1.4e-6
The normalised cross products of depth differences and the division by the opacity were expected to raise some of these above
the floor. They do not on these frames: the surface under the kept pixels is covered (opacity well above the clamp), and a
pixel whose cross product is short against the differences it is made of is out of keep_n. 2 e32 is at most 6.6e-6, every GPU
bound is at the 2e-4 floor and BOUNDS stays empty (on the GPU the worst array sits at 0.06 of its bound: proj of 2dgs-inria,
1.2e-5; tests/test_gpu_step_geometry.py).

3. The cuts: every new one moves a named array by at least ten bounds on every case it applies to. Per cut, the largest move
among its arrays, smallest over the cases, in bounds (2e-4 of the array's largest entry):
  distortion_geometry 2139 (xyz, pose-distortion-median), distortion_values 497 (xyz, 2dgs-gscuda-median; view by 1690 on the
  pose case), normal_rotation 1753 (rotation), normal_weights 2444, depth_normal_opacity 29338 (xyz, 2dgs-inria alone),
  depth_normal_weight 1028 (the WRONG form: opacity differentiated in the depth normal's weight), median_values 890 (xyz,
  2dgs-gscuda-median; view by 3825 on the pose case)
The terms' shares (lam_d, lam_n of step_frames.LAMBDA): the largest entry of the distortion term's xyz.grad / rotation.grad over
the colour's is 0.31 / 3.29 on 2dgs-inria and 0.25 / 0.85 on 2dgs-gscuda-median; the consistency term's 0.72 / 2.15 and 1.95 / 0.74.

4. The frames: 2dgs-inria 836 of 960 pixels with a depth normal; 2dgs-gscuda-median 438, and 529 select a median id; pose-
distortion-median 944 select one (16 blend nothing); 51 .. 55 of the 118 .. 126 visible normals are flipped, every axis is the
shortest of at least 31 rows.
"""
import functools
import os

import numpy as np
import pytest

import step_autograd_ref as R
import step_frames as S
from step_frames import BG, GEOMETRY_CASES, H, N, W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CAMERA = ("view", "proj", "cam_pos")
GEOMETRY = ("xyz", "opacity_logit", "log_scale", "rotation")


def _arrays(case):
    c = GEOMETRY_CASES[case]
    cam = tuple(k for k in CAMERA if k not in c["constant"])
    extra = (("features",) if c["channels"] else ()) + (("distortion_values",) if c["distortion"] == "values" else ()) \
        + (("median_values",) if c["median"] == "values" else ())
    return R.RAW + extra + cam


def _values32(case, which, scene, cam):
    """The float32 values the distortion / median pass is handed: the view depth as autograd forms it, or the scene's tensor."""
    import walk_ref
    kind = GEOMETRY_CASES[case][which]
    if kind is None:
        return None
    return walk_ref.depth_values(scene["means3D"], cam.view) if kind == "depth" else S.geometry_scene(case)[which + "_values"]


@functools.lru_cache(maxsize=None)
def frame(case):
    """The case's frame on the CPU: the float32 arrays the oracle is fed, the oracle's forward state, the float32 maps of the
    references of each pass, the structure with every decision, and the float64 reference step."""
    import features_ref
    import median_ref
    import walk_ref
    from oracle import cpu_oracle, inria_np
    c = GEOMETRY_CASES[case]
    raw, cam = S.geometry_scene(case), S.geometry_camera_of(case)
    act = S.activated_scene(raw)
    rows = S.geometry_row_arrays(case, act["scales"], act["opacities"], act["means3D"], act["rotations"], cam)
    scene = dict(act, scales=rows["scales"], opacities=rows["opacities"])
    if c["profile"] == "inria":
        st = inria_np.forward(scene, cam, BG, deg=c["sh_degree"], scale_modifier=c["scale_modifier"], blend_with="numpy-expf")
    else:
        st = cpu_oracle.forward(scene, cam, BG, scale_modifier=c["scale_modifier"])
    cutoff = walk_ref.T_CUTOFF[c["profile"]]
    med = None
    if c["median"]:
        med = median_ref.forward(st["means2D"], st["conicOpacity"], st["ranges"], st["values"], _values32(case, "median", scene, cam),
                                 W, H, c["threshold"], cutoff)
    structure = S.geometry_structure_of(case, cam, rows, st["radii"], st["ranges"], st["values"], st["nContrib"], st.get("clamped"),
                                        med["ids"] if med else None)
    maps32 = {"opacity": (np.float32(1.0) - st["finalT"].astype(np.float32)).astype(np.float32), "median": med["out"] if med else None}
    if c["depth"]:
        z = walk_ref.depth_values(scene["means3D"], cam.view)
        maps32["depth"] = features_ref.forward(st, z[:, None], None, W, H, t_cutoff=cutoff)["out"][0]
    surface32 = S.surface_of(case, maps32.get("depth"), maps32["opacity"], maps32["median"]) if c["surface"] else None
    grads, color, dmap, aux, drop, keep_n = S.geometry_reference_step(case, structure, surface32)
    return dict(case=case, raw=raw, cam=cam, scene=scene, act=act, rows=rows, st=st, structure=structure, drop=drop, keep_n=keep_n,
                grads=grads, color=color, dmap=dmap, aux=aux, med=med, maps32=maps32, surface32=surface32, cutoff=cutoff)


def _share(got, want):
    scale = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, np.float64) - want).max()) / scale if scale > 0 else float(np.abs(got).max())


@functools.lru_cache(maxsize=None)
def _step(case, cut=None, dtype=R.F64, only=None, colour=True):
    f = frame(case)
    return S.geometry_reference_step(case, f["structure"], f["surface32"], cut=cut, dtype=dtype, drop=f["drop"], keep_n=f["keep_n"],
                                     only=only, colour=colour)[0]


# ---- 1. the forward is the references' --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(GEOMETRY_CASES))
def test_restated_maps_are_the_references(case):
    import distortion_ref
    import features_ref
    import normals_ref
    from helpers import image_report
    f, c = frame(case), GEOMETRY_CASES[case]
    st, keep, aux = f["st"], ~f["drop"], f["aux"]
    assert ((aux["last"] == st["nContrib"]) | f["drop"]).all()
    report = {"image": image_report(f["color"] * keep, st["out_color"] * keep), "finalT": image_report(aux["finalT"] * keep, st["finalT"] * keep)}
    if c["opacity"]:
        report["opacity"] = image_report(aux["opacity_map"] * keep, f["maps32"]["opacity"] * keep)
    if c["depth"]:
        report["depth"] = image_report(f["dmap"] * keep, f["maps32"]["depth"] * keep)
    if c["distortion"]:
        d32 = distortion_ref.forward32(st, _values32(case, "distortion", f["scene"], f["cam"]), c["power"], W, H, t_cutoff=f["cutoff"])
        assert (d32["nContrib"] == st["nContrib"]).all()
        report["distortion"] = image_report(aux["distortion_map"] * keep, d32["out"] * keep)
    if c["median"]:
        report["median"] = image_report(aux["median_map"] * keep, f["med"]["out"] * keep)
        assert ((aux["median_selected"] == f["structure"]["median_ids"]) | f["drop"]).all()          # ids: exact on every kept pixel
    if c["normals"]:
        n32 = normals_ref.gaussian_normals_f32(f["scene"]["means3D"], f["scene"]["scales"], f["scene"]["rotations"], f["cam"].view, c["profile"])[0]
        replay = features_ref.forward(st, n32, None, W, H, t_cutoff=f["cutoff"])
        report["normals"] = image_report(aux["normal_map"] * keep, replay["out"] * keep)
    if c["channels"]:
        feat = features_ref.forward(st, f["raw"]["features"][:, :c["channels"]], None, W, H, t_cutoff=f["cutoff"])
        report["features"] = image_report(aux["feature_map"] * keep, feat["out"] * keep)
    print(f"[step geometry] {case}: " + ", ".join(f"{k} worst {v[0]:.1e}" for k, v in report.items())
          + f"; {int(f['drop'].sum())} pixels dropped")
    assert all(v[1] == 0 for v in report.values()), (case, {k: v[:2] for k, v in report.items()})


FD_ENTRIES = 2                   # per array: the entries of the largest gradient, on different rows
FD_STEP, FD_TOL = 1e-6, 1e-6     # tests/test_backward_oracle.py's: |g - fd| <= 1e-6 max(1, max |fd|)


@pytest.mark.parametrize("case", ["2dgs-inria", "pose-distortion-median"])
def test_reference_gradient_is_the_central_difference_of_its_own_loss(case):
    import torch
    f, c = frame(case), GEOMETRY_CASES[case]
    cam, g = f["cam"], S.geometry_weights(case)
    consistency = None
    if c["surface"]:
        import normals_ref
        # opacity.detach() is a constant of the differentiated function: the differences hold it at this frame's value
        consistency = dict(decisions=normals_ref.depth_normals_f32(f["surface32"], (cam.tan_fovx, cam.tan_fovy), c["profile"])[1],
                           keep_n=f["keep_n"], opacity_weight=f["aux"]["opacity_map"])
    terms = S.geometry_loss_terms(case, consistency)

    def loss_at(name, index, delta):
        leaf = S.geometry_leaves(case)
        with torch.no_grad():
            leaf[name].reshape(-1)[index] += delta
        return R.gradients(leaf, f["structure"], cam, g["w"], g["wd"], f["drop"], wf=g["wf"], loss_terms=terms, loss_only=True,
                           **S.geometry_forward_options(case))
    got, fd = [], []
    for name in ("xyz", "rotation") + (("view",) if "view" not in c["constant"] else ()):
        grad = f["grads"][name].reshape(-1)
        width = f["grads"][name].shape[-1] if f["grads"][name].ndim > 1 else 1
        order, rows = np.argsort(-np.abs(grad)), set()
        for i in order:
            if i // width not in rows:
                rows.add(i // width)
                got.append(grad[i])
                fd.append((loss_at(name, int(i), FD_STEP) - loss_at(name, int(i), -FD_STEP)) / (2.0 * FD_STEP))
                print(f"[step geometry] {case}: {name}[{i}] autograd {grad[i]:.9e}, central difference {fd[-1]:.9e}")
            if len(rows) == FD_ENTRIES:
                break
    got, fd = np.array(got), np.array(fd)
    assert np.abs(got - fd).max() <= FD_TOL * max(1.0, np.abs(fd).max()), (case, got, fd)


# ---- 2. the float32 noise floor ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(GEOMETRY_CASES))
def test_float32_noise_floor_sets_the_gpu_bounds(case):
    f = frame(case)
    g32 = _step(case, None, R.F32)
    line = []
    for k in _arrays(case) + ("mean2D",):
        key = "per_gaussian.mean2D" if k == "mean2D" else k
        want = f["grads"][key]
        if np.abs(want).max() == 0:
            assert (case, k) not in R.BOUNDS, (case, k)
            continue
        e32 = _share(g32[key], want)
        b = R.bound(case, k)
        line.append(f"{k} {e32:.1e}")
        assert b == R.FLOOR or 2 * e32 <= b <= 10 * e32, (case, k, e32, b)
        assert b >= 2 * e32, (case, k, e32, b)
    print(f"[step geometry] {case}: e32: " + ", ".join(line))


# ---- 3. the cuts are seen, the terms weigh alike ----------------------------------------------------------------------------
def cuts_of(case):
    """The new cuts that apply to a case -> the arrays of which at least one must move by at least ten bounds."""
    c = GEOMETRY_CASES[case]
    leaf_view = ("view",) if "view" not in c["constant"] else ()
    out = {}
    if c["distortion"]:
        out["distortion_geometry"] = GEOMETRY
        out["distortion_values"] = ("xyz",) + leaf_view if c["distortion"] == "depth" else ("distortion_values",)
    if c["normals"]:
        out["normal_rotation"] = ("rotation",)
        out["normal_weights"] = ("xyz", "opacity_logit", "log_scale")
    if c["surface"] == "expected":
        out["depth_normal_opacity"] = GEOMETRY
    if c["surface"]:
        out["depth_normal_weight"] = GEOMETRY
    if c["median"]:
        out["median_values"] = ("xyz",) + leaf_view if c["median"] == "depth" else ("median_values",)
    return out


SEEN = 10.0


@pytest.mark.parametrize("case", list(GEOMETRY_CASES))
def test_every_new_cut_is_seen(case):
    f = frame(case)
    unseen = []
    for cut, arrays in cuts_of(case).items():
        g = _step(case, cut)
        moved = {k: _share(g[k], f["grads"][k]) / R.bound(case, k) for k in arrays}
        print(f"[step geometry] {case}: cut {cut} moves " + ", ".join(f"{k} by {v:.0f} bounds" for k, v in moved.items()))
        if not max(moved.values()) >= SEEN:
            unseen.append((cut, moved))
        assert all(np.isfinite(g[k]).all() for k in _arrays(case))
    assert not unseen, (case, unseen)


def test_every_new_cut_applies_somewhere():
    new = R.CUTS[R.CUTS.index("distortion_geometry"):]
    assert set(new) == set().union(*(cuts_of(case) for case in GEOMETRY_CASES)), new


@pytest.mark.parametrize("case", [k for k, c in GEOMETRY_CASES.items() if c["surface"]])
def test_the_regularisers_weigh_like_the_colour(case):
    """lam_d and lam_n: each term's largest entry of xyz.grad and of rotation.grad is between a tenth and ten times the colour
    term's — a cut must move the array, and a bound is a share of the array's largest entry."""
    colour = _step(case, only=())
    for term in ("distortion", "consistency"):
        g = _step(case, only=(term,), colour=False)
        shares = {k: float(np.abs(g[k]).max() / np.abs(colour[k]).max()) for k in ("xyz", "rotation")}
        print(f"[step geometry] {case}: the {term} term's largest entry over the colour's: " + ", ".join(f"{k} {v:.2f}" for k, v in shares.items()))
        assert all(0.1 <= v <= 10.0 for v in shares.values()), (case, term, shares)


# ---- 4. conditions on the frames and the caps -------------------------------------------------------------------------------
def assert_caps(case, drop, keep_n, aux, structure, cam, surface_normal):
    """The caps of a GEOMETRY_CASES frame, on the CPU oracle's state here and on the device's arrays in the GPU test: returns
    (dropped, eroded) pixel counts. surface_normal: the float32 depth normal [3,H,W] of the case's surface (None: no term)."""
    c = GEOMETRY_CASES[case]
    assert drop.sum() <= 0.01 * W * H, int(drop.sum())
    lost = 0
    if c["surface"]:
        lost = int((~keep_n & ~drop).sum())
        assert lost <= 0.05 * W * H, lost
        assert (np.abs(surface_normal).max(0) > 0).sum() >= 0.25 * W * H, int((np.abs(surface_normal).max(0) > 0).sum())
    near, differ = R.rows_near_a_threshold(aux, structure, cam.tan_fovx, cam.tan_fovy, S.geometry_filter_values(case), c["antialiased"],
                                           c["normals"])
    assert not near.any() and not differ.any(), (case, np.nonzero(near)[0], np.nonzero(differ)[0])
    if c["median"]:
        ids = structure["median_ids"]
        assert (ids >= 0).sum() >= 0.1 * W * H and (ids < 0).any(), (int((ids >= 0).sum()), int((ids < 0).sum()))
    return int(drop.sum()), lost


@pytest.mark.parametrize("case", list(GEOMETRY_CASES))
def test_frame_conditions(case):
    import normals_ref
    f, c = frame(case), GEOMETRY_CASES[case]
    s, aux = f["structure"], f["aux"]
    vis = s["vis"]
    assert vis.sum() >= N / 2 and (~vis).sum() >= N / 8, (int(vis.sum()), N)
    normal = normals_ref.depth_normals_f32(f["surface32"], (f["cam"].tan_fovx, f["cam"].tan_fovy), c["profile"])[0] if c["surface"] else None
    dropped, lost = assert_caps(case, f["drop"], f["keep_n"], aux, s, f["cam"], normal)
    line = f"[step geometry] {case}: {dropped} pixels dropped, {lost} more without the consistency term"
    if c["surface"]:
        line += f", {int((np.abs(normal).max(0) > 0).sum())} of {W * H} with a depth normal"
    if c["median"]:
        line += f", {int((s['median_ids'] >= 0).sum())} select a median id"
    if c["normals"]:
        dec = s["normal_decisions"]
        line += f", {int(dec['flipped'][vis].sum())} of {int(vis.sum())} normals flipped, axes {np.bincount(dec['axis'][vis], minlength=3).tolist()}"
        assert dec["valid"][vis].all() and 0 < dec["flipped"][vis].sum() < vis.sum() and (np.bincount(dec["axis"][vis], minlength=3) > 0).all()
    print(line)
    for k in _arrays(case)[:4]:
        rows = np.abs(f["grads"][k].reshape(N, -1)).max(1) > 0
        assert rows.sum() >= N / 4, (k, int(rows.sum()))
    if not c["colour"]:
        assert (f["grads"]["shs"] == 0).all()
    for k in ("distortion_values", "median_values"):
        if k in _arrays(case):
            assert (np.abs(f["grads"][k]) > 0).sum() >= 10, k


# ---- 5. the earlier cases are untouched -------------------------------------------------------------------------------------
RECORDED_HOST = "3585da7f7793f44a"       # _host_arithmetic() of the host that recorded the two arrays
SAME_VALUES = 1e-12        # elsewhere: float64 rounding (1.1e-16) over the few thousand operations of a chain, with a margin of ten


def _host_arithmetic():
    """A digest of the bits this host gives a fixed float64 computation in the operations the reference is made of (torch's
    matrix products in the reference's shapes, batched and transposed; exp, sqrt, cumprod, sums). Two hosts whose math
    libraries round these differently cannot give each other's bits for the reference either."""
    import hashlib
    import torch
    rng = np.random.default_rng(5)
    t = lambda *shape: torch.from_numpy(rng.normal(size=shape))
    a, v, P, Sg, c = t(126, 3), t(3, 3), t(126, 2, 3), t(126, 3, 3), t(40, 3)
    w = torch.from_numpy(rng.uniform(0.0, 0.9, size=(40, 256)))
    cov = P @ (Sg @ Sg.transpose(1, 2)) @ P.transpose(1, 2)
    parts = [a @ v.T + v[2], cov, torch.exp(-w * w), torch.cumprod(1.0 - w, 0), w.T @ c, w @ (w.T @ c), torch.sqrt(w).sum(0),
             (w * torch.exp(-w)).sum(1), torch.prod(1.0 - w, 0), a / torch.sqrt((a * a).sum(1, keepdim=True)), 1.0 / (1.0 + torch.exp(-a))]
    return hashlib.sha256(b"".join(np.ascontiguousarray(x.numpy()).tobytes() for x in parts)).hexdigest()[:16]


def test_the_old_cases_give_the_parent_commits_bits():
    """forward() and gradients() with every new option at its default: the reference of CASES and of FULL_CASES is, bit for bit,
    the one recorded before the options were added (tests/golden/step_reference_*.npy: float64, one array of one case each).
    Bits of a float64 torch computation are a host's: where this host's arithmetic is not the recording's (_host_arithmetic —
    a digest that owes nothing to the reference) the same values are asserted instead, to SAME_VALUES of the largest entry."""
    import test_step_autograd_cpu as old
    import test_step_full_cpu as full
    f = old.frame("inria-3-depth")
    assert not {"normal_decisions", "median_ids"} & set(f["structure"])
    assert not {"distortion_map", "normal_map", "median_map"} & set(f["aux"])
    same_host = _host_arithmetic() == RECORDED_HOST
    print(f"[step geometry] the recording's arithmetic: {same_host} ({_host_arithmetic()})")
    for got, name in ((f["grads"]["rotation"], "step_reference_inria-3-depth_rotation.npy"),
                      (full.frame("full-inria")["grads"]["log_scale"], "step_reference_full-inria_log_scale.npy")):
        want = np.load(os.path.join(GOLDEN, name))
        assert got.dtype == want.dtype and got.shape == want.shape, name
        if same_host:
            assert np.array_equal(got, want), (name, float(np.abs(got - want).max()))
        else:
            assert _share(got, want) <= SAME_VALUES, (name, _share(got, want))
