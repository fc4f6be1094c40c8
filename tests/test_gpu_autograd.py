"""GPU: gsrast_amd.autograd — the activation kernels against the .ply loader and the float64 reference
(tests/activation_ref.py), `render(...)` + `loss.backward()` against the hand-run draw() + backward() and the CPU oracle, the
camera gradients, the ownership rules (no aliasing between steps, a stale graph refused) and a short training loop.

The scene: 160 Gaussians (scenes.garden_like_scene drawn smaller, its splats four times larger so that they cover pixels)
on 64 x 48 pixels: 4 x 3 tiles of 16 x 16; 160 Gaussians are two whole waves and a partial one."""
import functools

import numpy as np
import pytest

import activation_ref as A
from test_gpu_backward_poses import BG, RTOL, _check_chain, _close, _expected_chain, _state

pytestmark = pytest.mark.gpu

W, H, N = 64, 48, 160
DRAW = dict(plan="sort", tile_history=False)
RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")


def _cam(which=1):
    from helpers import posed_camera
    pose = {1: dict(eye=(2.0, -1.2, -4.2), target=(0.0, 0.0, 0.0), roll=0.4),
            2: dict(eye=(-1.5, 2.0, 3.5), target=(0.2, 0.0, 0.0), roll=-0.7)}[which]
    return posed_camera(W, H, **pose)


@functools.lru_cache(maxsize=None)
def _raw_scene(profile, n=N, seed=4):
    """Raw values of the scene: log of its scales, logit of its opacities, its quaternions at lengths 0.5 .. 2. The upstream
    profile with all sixteen SH triples, coefficient-major."""
    from gsrast_amd import scenes
    sc = scenes.garden_like_scene(n, seed=seed)
    rng = np.random.default_rng(seed)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-4, 1.0 - 1e-4)
    raw = {"xyz": (sc["means3D"][:, :3] * 0.25).astype(np.float32),
           "opacity_logit": np.log(o / (1.0 - o)).astype(np.float32),
           "log_scale": np.log(4.0 * sc["scales"][:, :3].astype(np.float64)).astype(np.float32),
           "rotation": (sc["rotations"] * rng.uniform(0.5, 2.0, (n, 1))).astype(np.float32),
           "shs": sc["shs"].astype(np.float32)}
    if profile == "inria":
        raw["shs"] = rng.normal(0, 0.35, (n, 48)).astype(np.float32)
    return raw


def _params(profile, requires=RAW):
    from gsrast_amd.autograd import GaussianParams
    raw = _raw_scene(profile)
    p = GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if profile == "inria" else "file",
                                device="cuda:0")
    for k in RAW:
        getattr(p, k).requires_grad_(k in requires)
    return p


def _rasterizer():
    from gsrast_amd.rasterizer import SplatRasterizer
    return SplatRasterizer(W, H, background=BG)


def _weights(seed=17):
    """Seeded loss weights: white noise on the colour; on the depth a smooth field of one sign, as a depth loss gives it
    (tests/test_gpu_backward_poses.py, the depth term)."""
    import torch
    rng = np.random.default_rng(seed)
    w = rng.normal(size=(3, H, W)).astype(np.float32)
    wd = (1.0 + 0.25 * rng.normal(size=(H, W))).astype(np.float32)
    return torch.from_numpy(w).cuda(), torch.from_numpy(wd).cuda(), w, wd


def _kw(profile):
    return dict(semantics=profile, sh_degree=3)


def _bits(t):
    import torch
    t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and bool((_bits(a) == _bits(b)).all())


def _step(profile, params, rast, cam, depth):
    """One training step's forward and backward: the loss is (w . color).sum() + (wd . depth).sum()."""
    from gsrast_amd.autograd import render
    wt, wdt, _, _ = _weights()
    color, dmap, opacity = render(params, rast, cam, depth=depth, **_kw(profile), **DRAW)
    loss = (wt * color).sum()
    if depth:
        loss = loss + (wdt * dmap).sum()
    loss.backward()
    return color, dmap, opacity


# ---- 1. the activation forward ---------------------------------------------------------------------------------------------
def _records(n, seed):
    """62-float records with ordinary raw values and, where n leaves room (a later one replaces an earlier one in the same
    row), logits +-90, log-scales -100 and 88 and one zero quaternion."""
    rng = np.random.default_rng(seed)
    rec = rng.normal(size=(n, 62)).astype(np.float32)
    rec[:, 54] = rng.uniform(-6, 6, n)
    rec[:, 55:58] = rng.uniform(-6, 2, (n, 3))
    rec[:, 58:62] *= rng.uniform(0.3, 3.0, (n, 1)).astype(np.float32)
    rec[0 % n, 54] = 90.0
    rec[1 % n, 54] = -90.0
    rec[2 % n, 55] = -100.0
    rec[3 % n, 56] = 88.0
    rec[4 % n, 58:62] = 0.0
    return rec


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_activation_forward_is_the_ply_loaders_bit_for_bit(n):
    import torch
    from gsrast_amd import _capi
    from gsrast_amd.autograd import activate
    L = _capi.lib()
    rec = _records(n, 100 + n)
    dev = torch.device("cuda:0")
    raw = torch.from_numpy(rec).to(dev)
    want = [torch.empty((n, 4), dtype=torch.float32, device=dev) for _ in range(3)] + [torch.empty((n,), dtype=torch.float32, device=dev)]
    shs = torch.empty((n, 48), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _capi.check(L.gsr_ply_activate_layout(raw.data_ptr(), n, *(t.data_ptr() for t in want), shs.data_ptr(),
                                          _capi.GSR_SH_LAYOUT_FILE, stream), "gsr_ply_activate_layout")
    got = activate(raw[:, 0:3].clone(), raw[:, 54].clone(), raw[:, 55:58].clone(), raw[:, 58:62].clone())
    torch.cuda.synchronize()
    for name, g, w in zip(("means3D", "scales", "rotations", "opacities"), got, want):
        assert _same_bits(g, w), name
    if n > 4:
        o, s, q = (t.cpu().numpy() for t in (got[3], got[1], got[2]))
        assert o[0] == 1.0 and o[1] < 1e-38 and s[2, 0] < 1e-38 and np.isfinite(s[3, 1]) and s[3, 1] > 1e38 and np.isnan(q[4]).all()
        assert (s[:, 3] == np.float32(np.e)).all() and (got[0][:, 3] == 1.0).all()


# ---- 2. the activation backward --------------------------------------------------------------------------------------------
def _backward_case(n, seed):
    """Raw values and incoming gradients whose results are normal floats (the bound is relative): logits in [-8, 8] and +-30,
    log-scales in [-8, 4] and -20, 10, quaternions of length 0.3 .. 3, gradients over six decades."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-8, 8, n).astype(np.float32)
    s = rng.uniform(-8, 4, (n, 3)).astype(np.float32)
    r = rng.normal(size=(n, 4))
    r = (r * rng.uniform(0.3, 3.0, (n, 1)) / np.linalg.norm(r, axis=1, keepdims=True)).astype(np.float32)
    x[0 % n], x[1 % n], s[2 % n, 0], s[3 % n, 2] = 30.0, -30.0, -20.0, 10.0
    g = [(rng.normal(size=(n, 4)) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32) for _ in range(4)]
    radii = rng.integers(-1, 3, n).astype(np.int32)          # about half culled (0 and -1)
    return x, s, r, g, radii


def _run_backward(n, x, s, r, g, radii=None, outputs=(0, 1, 2, 3), drop_unused_inputs=False):
    """gsr_activate_params_backward through ctypes into one sentinel-filled arena: the four outputs with gaps between them.
    Returns (outputs as numpy or None where not asked for, the arena as float32 numpy, the slices)."""
    import torch
    from gsrast_amd import _capi
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    xt, st, rt = up(x), up(s), up(r)
    gt = [up(a) for a in g]
    rad = up(radii) if radii is not None else None
    sizes = (3 * n, n, 3 * n, 4 * n)
    gap = 64
    starts, at = [], gap
    for k in sizes:
        starts.append(at)
        at += (k + 3) // 4 * 4 + gap                          # (every output starts on a 16-byte boundary)
    SENTINEL = -7.0
    arena = torch.full((at,), SENTINEL, dtype=torch.float32, device=dev)
    sl = [slice(a, a + k) for a, k in zip(starts, sizes)]
    outp = [arena[q].data_ptr() if i in outputs else None for i, q in enumerate(sl)]
    used = lambda i, t: t.data_ptr() if (i in outputs or not drop_unused_inputs) else None
    rc = _capi.lib().gsr_activate_params_backward(
        n, used(1, xt), used(2, st), used(3, rt), rad.data_ptr() if rad is not None else None,
        used(0, gt[0]), used(2, gt[1]), used(3, gt[2]), used(1, gt[3]), *outp, torch.cuda.current_stream(dev).cuda_stream)
    _capi.check(rc, "gsr_activate_params_backward")
    torch.cuda.synchronize()
    host = arena.cpu().numpy()
    shapes = ((n, 3), (n,), (n, 3), (n, 4))
    outs = [host[q].reshape(sh).copy() if i in outputs else None for i, (q, sh) in enumerate(zip(sl, shapes))]
    return outs, host, sl, SENTINEL


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_activation_backward_matches_the_float64_reference(n):
    x, s, r, g, radii = _backward_case(n, 200 + n)
    names = ("dL_draw_means", "dL_draw_opacity", "dL_draw_scales", "dL_draw_rotations")
    want = A.backward(x, s, r, g[0], g[1], g[2], g[3][:, 3])
    got, host, sl, sentinel = _run_backward(n, x, s, r, g)
    for name, a, w in zip(names, got, want):
        err, tol = np.abs(a.astype(np.float64) - w), A.tolerance(w)
        print(f"[activation backward] n={n} {name}: worst error {float((err / tol).max()):.3f} of the bound")
        assert np.isfinite(a).all() and (err <= tol).all(), (name, float((err / tol).max()))
    assert (got[0] == g[0][:, :3]).all()
    # the quaternion's gradient is orthogonal to the quaternion: each component is off by at most its bound, the dot
    # product of the float32 result with r (in float64) therefore by at most sum_k bound_k |r_k|
    dot = (got[3].astype(np.float64) * r.astype(np.float64)).sum(1)
    assert (np.abs(dot) <= (A.tolerance(want[3]) * np.abs(r.astype(np.float64))).sum(1)).all()
    # outside the four outputs nothing was written
    mask = np.ones(host.size, bool)
    for q in sl:
        mask[q] = False
    assert (host[mask] == sentinel).all()
    # radii: exact zeros for the culled rows, the same bits as without radii for the others
    cut, host_c, _, _ = _run_backward(n, x, s, r, g, radii=radii)
    off = radii <= 0
    for name, a, b in zip(names, cut, got):
        assert (a[off].view(np.uint32) == 0).all(), name
        assert (a[~off].view(np.uint32) == b[~off].view(np.uint32)).all(), name
    assert (host_c[mask] == sentinel).all()
    # every output alone, the inputs of the others NULL too: the same bits, and the others' buffers untouched
    for only in range(4):
        one, host_1, sl_1, _ = _run_backward(n, x, s, r, g, radii=radii, outputs=(only,), drop_unused_inputs=True)
        assert (one[only].view(np.uint32) == cut[only].view(np.uint32)).all(), names[only]
        keep = np.ones(host_1.size, bool)
        keep[sl_1[only]] = False
        assert (host_1[keep] == sentinel).all(), names[only]


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _end_to_end(profile):
    """One step through render() + loss.backward() (upstream profile: SH degree 3 and a depth term), the same frame by hand
    (activate, draw, backward with every output) on a rasterizer of its own, and that rasterizer's forward state."""
    import torch
    from gsrast_amd.autograd import activate
    depth = profile == "inria"
    cam = _cam(1)
    wt, wdt, w, wd = _weights()
    params = _params(profile)
    color, dmap, opacity = _step(profile, params, _rasterizer(), cam, depth)
    grads = {k: getattr(params, k).grad for k in RAW}
    with torch.no_grad():
        act = activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
    scene = {k: t.cpu().numpy() for k, t in zip(("means3D", "scales", "rotations", "opacities"), act)}
    scene["shs"] = params.shs.detach().cpu().numpy()
    r2 = _rasterizer()
    r2.configure_from_scene(scene)
    img = r2.draw(cam, depth=depth, **_kw(profile), **DRAW).cpu().numpy().copy()
    dimg = r2.out_depth.cpu().numpy().copy() if depth else None
    hand = {k: v.cpu().numpy().copy() for k, v in
            r2.backward(wt, dL_ddepth=wdt if depth else None, wide_sums=True, **_kw(profile)).items()}
    g, im, plist, clamped = _state(r2)
    torch.cuda.synchronize()
    return dict(profile=profile, depth=depth, cam=cam, params=params, color=color, dmap=dmap, opacity=opacity, grads=grads,
                scene=scene, r2=r2, img=img, dimg=dimg, hand=hand, g=g, im=im, plist=plist, clamped=clamped, w=w, wd=wd)


def _reference_raw_grads(f, per_gaussian):
    raw = _raw_scene(f["profile"])
    return A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], per_gaussian["dL_dmeans3D"], per_gaussian["dL_dscales"],
                      per_gaussian["dL_drotations"], per_gaussian["dL_dconic_opacity"][:, 3], radii=f["g"]["radii"])


@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_render_backward_matches_the_hand_run_path(profile):
    f = _end_to_end(profile)
    assert _same_bits(f["color"], f["img"])
    if f["depth"]:
        assert _same_bits(f["dmap"], f["dimg"])
    assert np.array_equal(f["opacity"].cpu().numpy(), 1.0 - f["im"]["finalT"]) and not f["opacity"].requires_grad
    want = dict(zip(("xyz", "opacity_logit", "log_scale", "rotation"), _reference_raw_grads(f, f["hand"])))
    want["shs"] = f["hand"]["dL_dshs"].astype(np.float64)
    for k in RAW:
        got = f["grads"][k].cpu().numpy().astype(np.float64)
        err, tol = np.abs(got - want[k]), A.tolerance(want[k])
        print(f"[autograd] {profile} {k}.grad: worst error {float((err / np.maximum(tol, 1e-300)).max()):.3f} of the bound")
        assert got.shape == want[k].shape and (err <= tol).all(), k
        assert np.abs(want[k]).max() > 0, k


@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_per_gaussian_gradients_of_the_function_match_the_oracle(profile):
    """rasterize() on leaf tensors: their .grad is what the Function got from gsr_backward. The sums against the float64
    blend backward, the chain per visible Gaussian against oracle/backward_np.py, at tests/test_gpu_backward_poses.py's
    tolerances. Guards, from the CPU oracles alone: half of the scene is visible, and every raw-parameter gradient has
    non-zero rows."""
    import torch
    from gsrast_amd.autograd import rasterize
    from oracle import backward_np as B
    from oracle import cpu_oracle, inria_np
    from test_depth_cpu import depth_mean_term, depth_values_f32
    f = _end_to_end(profile)
    cam, scene, g, hand, depth = f["cam"], f["scene"], f["g"], f["hand"], f["depth"]
    dev = torch.device("cuda:0")
    leaves = {k: torch.from_numpy(scene[k]).to(dev).requires_grad_(True) for k in ("means3D", "scales", "rotations", "opacities", "shs")}
    cam_t = [torch.from_numpy(np.asarray(a, np.float32).copy()).to(dev) for a in (cam.view, cam.proj, cam.cam_pos)]
    color, dmap, _ = rasterize(_rasterizer(), *leaves.values(), *cam_t, (cam.tan_fovx, cam.tan_fovy), depth=depth,
                               **_kw(profile), **DRAW)
    wt, wdt, w, wd = _weights()
    loss = (wt * color).sum() + ((wdt * dmap).sum() if depth else 0.0)
    loss.backward()
    fn = {k: t.grad.cpu().numpy() for k, t in leaves.items()}
    assert _same_bits(color, f["img"])
    # the CPU oracle's own view of the frame: at least half of the Gaussians have a tile
    radii = (inria_np.preprocess(scene, cam, deg=3) if profile == "inria" else cpu_oracle.forward(scene, cam))["radii"]
    assert (np.asarray(radii) > 0).sum() >= N / 2
    vis = np.nonzero(g["radii"] > 0)[0]
    assert vis.size >= N / 2
    # the sums: the float64 blend backward over the forward state
    ranges = f["im"]["ranges"].view(np.uint32).astype(np.int64)
    cut = 1e-4 if profile == "inria" else 0.001
    out64, ft64, nc64 = B.blend_forward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, f["plist"], W, H, BG, t_cutoff=cut)
    assert np.abs(out64 - f["img"]).max() <= 1e-4
    exp = B.blend_backward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, f["plist"], nc64, ft64, W, H, BG, w)
    keys = ("dL_dmean2D", "dL_dconic", "dL_dopacity", "dL_dcolor")
    total = {k: exp[k].copy() for k in keys}
    term = np.zeros((N, 3))
    if depth:
        d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), False).astype(np.float64)
        g3 = np.zeros((3, H, W))
        g3[0] = wd
        exp_d = B.blend_backward(g["means2D"], g["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), ranges, f["plist"], nc64, ft64,
                                 W, H, (0.0, 0.0, 0.0), g3)
        for k in ("dL_dmean2D", "dL_dconic", "dL_dopacity"):
            total[k] += exp_d[k]
        _close(hand["dL_ddepths"], exp_d["dL_dcolor"][:, 0], "dL_ddepths")
        term = depth_mean_term(scene["means3D"][:, :3], np.asarray(cam.view, np.float32), hand["dL_ddepths"], False)
    _close(fn["opacities"], total["dL_dopacity"], "opacities.grad", RTOL)
    _close(hand["dL_dmean2D"], total["dL_dmean2D"], "dL_dmean2D", RTOL)
    _close(hand["dL_dconic_opacity"][:, :3], total["dL_dconic"], "dL_dconic", RTOL)
    _close(hand["dL_dcolors"], total["dL_dcolor"], "dL_dcolors", RTOL)
    # the chain: the Function's outputs in place of the hand-run call's, fed with that call's sums
    chain = dict(hand)
    chain["dL_dmeans3D"] = fn["means3D"].copy()
    chain["dL_dmeans3D"][:, :3] -= term
    chain["dL_dscales"], chain["dL_drotations"], chain["dL_dshs"] = fn["scales"], fn["rotations"], fn["shs"]
    e = _expected_chain(profile, chain, g, scene, cam, vis, f["clamped"])
    mags = _check_chain(profile, chain, g, scene, cam, vis, f["clamped"], expected=e)
    assert all(m > 0 for m in mags)
    culled = g["radii"] <= 0
    for k in ("means3D", "scales", "rotations", "opacities", "shs"):
        assert (fn[k][culled] == 0).all(), k
    if profile == "gscuda":
        assert (fn["shs"][:, 3:] == 0).all() and np.abs(fn["shs"][:, :3]).max() > 0
    # blindness guard on the oracle's expectation: every raw-parameter gradient has non-zero rows
    full = {k: np.zeros((N, 4)) for k in ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dconic_opacity")}
    full["dL_dmeans3D"][vis, :3] = e["dL_dmeans3D"] + term[vis]
    full["dL_dscales"][vis, :3] = e["dL_dscales"]
    full["dL_drotations"][vis] = e["dL_drotations"]
    full["dL_dconic_opacity"][:, 3] = total["dL_dopacity"]
    for name, a in zip(("xyz", "opacity_logit", "log_scale", "rotation"), _reference_raw_grads(f, full)):
        rows = np.abs(a.reshape(N, -1)).max(1) > 0
        assert rows.sum() >= N / 4, (name, int(rows.sum()))
    sh_rows = np.abs(e["dL_dshs"]).max(1) > 0 if profile == "inria" else np.abs(total["dL_dcolor"][vis]).max(1) > 0
    assert sh_rows.sum() >= N / 4


# ---- 4. the camera ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_camera_gradients_are_those_of_backward_camera(profile):
    import torch
    from gsrast_amd.autograd import render
    f = _end_to_end(profile)
    cam, depth = f["cam"], f["depth"]
    wt, wdt, _, _ = _weights()
    dev = torch.device("cuda:0")
    view, proj, pos = (torch.from_numpy(np.asarray(a, np.float32).copy()).to(dev).requires_grad_(True)
                       for a in (cam.view, cam.proj, cam.cam_pos))
    params = _params(profile)
    color, dmap, _ = render(params, _rasterizer(), (view.reshape(4, 4), proj, pos, cam.tan_fovx, cam.tan_fovy), depth=depth,
                            **_kw(profile), **DRAW)
    ((wt * color).sum() + ((wdt * dmap).sum() if depth else 0.0)).backward()
    r2 = f["r2"]
    r2.draw(cam, depth=depth, **_kw(profile), **DRAW)
    want = r2.backward(wt, dL_ddepth=wdt if depth else None, wide_sums=True, camera=True, **_kw(profile))
    assert _same_bits(color, f["img"])
    for t, k in ((view, "dL_dview_matrix"), (proj, "dL_dproj_matrix"), (pos, "dL_dcam_pos")):
        assert t.grad is not None and t.grad.shape == t.shape and _same_bits(t.grad.reshape(-1), want[k]), k
        # (the reference's profile does not read cam_pos: no gradient there)
        assert float(want[k].abs().max()) > 0 or (k == "dL_dcam_pos" and profile == "gscuda"), k
    for k in RAW:                                           # ... and the parameters' gradients are those of the step without
        assert _same_bits(getattr(params, k).grad, f["grads"][k]), k


# ---- 5. a subset of the inputs ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_only_the_inputs_that_require_a_gradient_get_one(profile):
    f = _end_to_end(profile)
    params = _params(profile, requires=("xyz",))
    _step(profile, params, _rasterizer(), f["cam"], f["depth"])
    for k in RAW[1:]:
        assert getattr(params, k).grad is None, k
    assert _same_bits(params.xyz.grad, f["grads"]["xyz"])


# ---- 6. no aliasing --------------------------------------------------------------------------------------------------------
def test_two_steps_share_no_memory():
    """Two steps on one rasterizer with different cameras and no clone in between: what step 1 returned — image, depth, every
    .grad — still holds step 1's values after step 2, as a third, separate run of step 1 computes them."""
    import torch
    profile = "inria"
    params, rast = _params(profile), _rasterizer()
    color1, depth1, opacity1 = _step(profile, params, rast, _cam(1), True)
    grads1 = {k: getattr(params, k).grad for k in RAW}
    for k in RAW:
        getattr(params, k).grad = None
    color2, depth2, _ = _step(profile, params, rast, _cam(2), True)
    torch.cuda.synchronize()
    fresh = _params(profile)
    color3, depth3, opacity3 = _step(profile, fresh, _rasterizer(), _cam(1), True)
    assert not _same_bits(color1, color2) and not _same_bits(depth1, depth2)          # (the second step drew another frame)
    assert _same_bits(color1, color3) and _same_bits(depth1, depth3) and _same_bits(opacity1, opacity3)
    for k in RAW:
        assert not _same_bits(grads1[k], getattr(params, k).grad), k
        assert _same_bits(grads1[k], getattr(fresh, k).grad), k
    ptrs = [t.data_ptr() for t in (color1, depth1, color2, depth2, rast.out_color)] + [g.data_ptr() for g in grads1.values()]
    ptrs += [getattr(params, k).grad.data_ptr() for k in RAW]
    assert len(set(ptrs)) == len(ptrs)


# ---- 7. a stale graph ------------------------------------------------------------------------------------------------------
def test_backward_of_a_frame_the_rasterizer_no_longer_holds_is_refused():
    import torch
    from gsrast_amd.autograd import render
    profile = "gscuda"
    wt, _, _, _ = _weights()
    params, rast = _params(profile), _rasterizer()
    color_a, _, _ = render(params, rast, _cam(1), **_kw(profile), **DRAW)
    color_b, _, _ = render(params, rast, _cam(2), **_kw(profile), **DRAW)
    with pytest.raises(RuntimeError, match="one rasterizer object per graph"):
        (wt * color_a).sum().backward()
    assert all(getattr(params, k).grad is None for k in RAW)
    (wt * color_b).sum().backward()
    torch.cuda.synchronize()
    fresh = _params(profile)
    color_c, _, _ = render(fresh, _rasterizer(), _cam(2), **_kw(profile), **DRAW)
    (wt * color_c).sum().backward()
    assert _same_bits(color_b, color_c)
    for k in RAW:
        assert _same_bits(getattr(params, k).grad, getattr(fresh, k).grad), k
        assert float(getattr(fresh, k).grad.abs().max()) > 0, k


# ---- 8. training -----------------------------------------------------------------------------------------------------------
def _train(steps=20):
    import torch
    from gsrast_amd.autograd import render
    profile = "inria"
    cam, rast = _cam(1), _rasterizer()
    with torch.no_grad():
        target = render(_params(profile), rast, cam, **_kw(profile))[0]
    params = _params(profile)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, amp in (("xyz", 0.02), ("opacity_logit", 0.5), ("log_scale", 0.2), ("rotation", 0.1), ("shs", 0.1)):
            p = getattr(params, k)
            p.add_((amp * torch.randn(p.shape, generator=gen)).to(p.device))
    # Adam moves a value by about its learning rate per step: each rate is a tenth to a twentieth of the perturbation above
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = torch.optim.Adam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        loss = (render(params, rast, cam, **_kw(profile))[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        if len(losses) <= steps:
            loss.backward()
            opt.step()
    return losses, [p.detach().clone() for p in params.parameters()]


def test_twenty_adam_steps_lower_the_loss_and_repeat_bit_for_bit():
    losses, end = _train()
    print(f"[training] L1 loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert losses[-1] < losses[0]
    losses2, end2 = _train()
    assert losses2 == losses
    for a, b in zip(end, end2):
        assert _same_bits(a, b)
