"""GPU: gradients w.r.t. the camera (backward(camera=True), gsr_camera_backward). Checked against the float64 reference
(tests/camera_grad_ref.py) applied to the library's own per-Gaussian gradients, end to end against the float64 blend
backward (oracle/backward_np.py), for bit reproducibility, for tile-row bands adding up to the frame, at the edges (nothing
visible, Gaussians behind the camera), on the 5.8 M-splat bench scene, and alone on synthetic per-Gaussian arrays at the sizes
where the pass's loops take further turns."""
import ctypes as C

import numpy as np
import pytest

from camera_grad_ref import ZERO_ENTRIES, camera_grad

pytestmark = pytest.mark.gpu

CAM_KEYS = ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")


def _setup(seed=2, w=100, h=70, n=1200, bg=(0.2, 0.5, 0.9)):
    """The scene of tests/test_gpu_depth_backward.py, with SH coefficients beyond the DC term (the upstream profile's
    colour then depends on the camera position)."""
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    scene = scenes.garden_like_scene(n, seed=seed)
    scene["means3D"][:, :3] *= 0.25
    scene["shs"][:, 3:] = 0.3 * np.random.default_rng(seed + 100).normal(size=(n, 45)).astype(np.float32)
    cam = camera.default_camera(w, h, near=0.05, far=50.0)
    r = SplatRasterizer(w, h, background=bg)
    r.configure_from_scene(scene)
    return r, scene, cam, bg


def _grads(cam, seed=11):
    import torch
    rng = np.random.default_rng(seed)
    dL = torch.from_numpy(rng.normal(size=(3, cam.height, cam.width)).astype(np.float32))
    gd = torch.from_numpy(rng.normal(size=(cam.height, cam.width)).astype(np.float32))
    return dL, gd


def _cam(out):
    return np.concatenate([np.asarray(out[k].cpu() if hasattr(out[k], "cpu") else out[k]) for k in CAM_KEYS])


def _clamped(r):
    import torch
    from gsrast_amd import _capi
    st = _capi.GeometryState()
    r.lib.gsr_geometry_from_chunk(r.geom.base(), r.num_gaussians, C.byref(st))
    return r.geom.view(st.clamped, 3 * r.num_gaussians, torch.uint8).cpu().numpy().reshape(-1, 3).astype(bool)


def _reference(r, cam, grads, semantics, mode, sh_degree, device="cpu"):
    """The float64 camera gradient of the per-Gaussian arrays `grads` (dL_dmean2D, dL_dcov2D, [dL_ddepths], [dL_dcolors])
    over the state of r's last draw()."""
    g = r.map_geometry_state()
    inria = semantics == "inria"
    return camera_grad(r.means3D, cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height,
                       g["radii"], g["cov3D"], grads["dL_dmean2D"], grads["dL_dcov2D"],
                       dL_ddepths=grads["dL_ddepths"] if mode else None, inverse=mode == "inverse", inria=inria,
                       shs=r.shs if inria else None, sh_degree=sh_degree, dL_dcolors=grads["dL_dcolors"] if inria else None,
                       clamped=_clamped(r) if inria else None, device=device)


def _assert_close(got, exp, M, what, rtol=1e-6):
    """|err_k| <= rtol M_k, plus 1e-12 of the largest M: an entry can vanish identically for every Gaussian — a camera at
    the origin makes cov2D invariant under the shears V[0][2], V[1][2] (pi(S t) = pi(t) + const) — and is then a sum of
    double rounding residues (~1e-17 each) that no two summation orders share."""
    assert np.isfinite(got).all(), what
    assert (got[ZERO_ENTRIES] == 0).all() and (got[M == 0] == 0).all(), f"{what}: entries without support are not zeros"
    err = np.abs(got.astype(np.float64) - exp)
    bad = err > rtol * M + 1e-12 * M.max()
    assert not bad.any(), f"{what}: entries {np.nonzero(bad)[0]}: err {err[bad]} > {rtol} x M {M[bad]}"


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


CASES = [(s, m, f, w) for s in ("gscuda", "inria") for m in (False, True, "inverse") for f in ("sorted", "block_lists")
         for w in (True, False)]


@pytest.mark.parametrize("semantics,mode,feed,wide", CASES)
def test_camera_grad_matches_the_reference_on_the_librarys_own_gradients(semantics, mode, feed, wide):
    """|err_k| <= 1e-6 M_k, M_k = sum_i |term_ik|, for the float64 reference applied to the arrays the same call returned."""
    r, scene, cam, bg = _setup()
    inria = semantics == "inria"
    sh_degree = 3 if inria else 0
    kw = dict(semantics=semantics, sh_degree=sh_degree, tile_history=False)
    if feed == "sorted":
        r.draw(cam, plan="sort", **kw)
    else:
        r.draw(cam, plan="blocks", sorted_lists=False, **kw)
        assert not r.last_lists_written
    dL, gd = _grads(cam)
    out = r.backward(dL, dL_ddepth=gd if mode else None, depth=mode or None, wide_sums=wide, semantics=semantics,
                     sh_degree=sh_degree, camera=True)
    assert set(CAM_KEYS) <= set(out) and out["dL_dview_matrix"].shape == (16,) and out["dL_dcam_pos"].shape == (3,)
    got = _cam(out)
    exp, M = _reference(r, cam, out, semantics, mode, sh_degree)
    what = f"{semantics}/{mode}/{feed}/wide={wide}"
    _assert_close(got, exp, M, what)
    assert M[:16].max() > 0 and M[16:32].max() > 0
    assert (M[32:] > 0).all() if inria else (got[32:] == 0).all(), what


def test_camera_grad_plumbing_of_outputs_and_with_cov3D():
    """backward(camera=True) makes gsr_backward write what the camera pass reads whatever `outputs` / `with_cov3D` say, and
    returns only what was asked for plus the three camera arrays; the camera gradient is the same either way."""
    r, scene, cam, bg = _setup()
    dL, gd = _grads(cam)
    r.draw(cam, plan="sort", tile_history=False)
    full = _cam(r.backward(dL, dL_ddepth=gd, camera=True))
    few = r.backward(dL, dL_ddepth=gd, camera=True, outputs=("dL_dcov3D",))
    assert sorted(few) == sorted(("dL_dcov3D", "dL_ddepths") + CAM_KEYS)
    assert np.array_equal(_bits(_cam(few)), _bits(full))
    bare = r.backward(dL, dL_ddepth=gd, camera=True, with_cov3D=False)
    assert "dL_dcov2D" not in bare and set(CAM_KEYS) <= set(bare)
    assert np.array_equal(_bits(_cam(bare)), _bits(full))
    plain = r.backward(dL, dL_ddepth=gd)
    assert not set(CAM_KEYS) & set(plain)


@pytest.mark.parametrize("semantics,mode", [("gscuda", False), ("gscuda", True), ("inria", "inverse")])
def test_camera_grad_end_to_end_against_the_float64_blend_backward(semantics, mode):
    """The camera gradient against the float64 reference applied to per-Gaussian gradients summed in float64 over the
    pixels (oracle/backward_np.py; the covariance gradient as -K dL/dK K of the float64 conic gradient): within 2e-4 of
    the largest entry."""
    from oracle import backward_np as B
    from test_depth_cpu import depth_values_f32
    r, scene, cam, bg = _setup()
    w, h = cam.width, cam.height
    inria = semantics == "inria"
    sh_degree = 3 if inria else 0
    r.draw(cam, plan="sort", semantics=semantics, sh_degree=sh_degree, tile_history=False)
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    plist = r.map_binning_state()["values"].cpu().numpy().view(np.uint32).astype(np.int64)
    dL, gd = _grads(cam)
    got = _cam(r.backward(dL, dL_ddepth=gd if mode else None, depth=mode or None, semantics=semantics, sh_degree=sh_degree,
                          camera=True))
    ranges = im["ranges"].view(np.uint32).astype(np.int64)
    _, ft64, nc64 = B.blend_forward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, w, h, bg,
                                    t_cutoff=1e-4 if inria else 0.001)
    assert (nc64 != im["nContrib"].view(np.uint32)).sum() <= 2
    e = B.blend_backward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, nc64, ft64, w, h, bg, dL.numpy())
    d_mean, d_conic, dd = e["dL_dmean2D"], e["dL_dconic"], None
    if mode:
        d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), mode == "inverse").astype(np.float64)
        g3 = np.zeros((3, h, w))
        g3[0] = gd.numpy()
        ed = B.blend_backward(g["means2D"], g["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), ranges, plist, nc64, ft64, w, h,
                              (0.0, 0.0, 0.0), g3)
        d_mean, d_conic, dd = d_mean + ed["dL_dmean2D"], d_conic + ed["dL_dconic"], ed["dL_dcolor"][:, 0]
    co = g["conicOpacity"].astype(np.float64)
    K = np.stack([np.stack([co[:, 0], co[:, 1]], 1), np.stack([co[:, 1], co[:, 2]], 1)], 1)
    gK = np.stack([np.stack([d_conic[:, 0], 0.5 * d_conic[:, 1]], 1), np.stack([0.5 * d_conic[:, 1], d_conic[:, 2]], 1)], 1)
    gM = -K @ gK @ K
    grads = {"dL_dmean2D": d_mean, "dL_dcov2D": np.stack([gM[:, 0, 0], gM[:, 0, 1], gM[:, 1, 1]], 1), "dL_ddepths": dd,
             "dL_dcolors": e["dL_dcolor"]}
    exp, M = _reference(r, cam, grads, semantics, mode, sh_degree)
    scale = float(np.abs(exp).max())
    err = float(np.abs(got - exp).max())
    assert scale > 0 and err <= 2e-4 * scale, f"{semantics}/{mode}: max abs err {err} at scale {scale}"


def test_camera_grad_is_bit_reproducible_and_leaves_the_other_outputs_alone():
    """wide_sums=True (the mode in which the backward itself is reproducible; sorted lists): two backward(camera=True) calls
    give the same bits, every other array equals backward(camera=False) bit for bit, and two camera passes over the same
    arrays give the same bits (both semantics)."""
    import torch
    r, scene, cam, bg = _setup(seed=5, w=128, h=96, n=4000)
    dL, gd = _grads(cam, seed=6)
    for semantics, sh_degree in (("gscuda", 0), ("inria", 3)):
        r.draw(cam, plan="sort", tile_history=False, semantics=semantics, sh_degree=sh_degree)
        kw = dict(dL_ddepth=gd, depth="inverse", semantics=semantics, sh_degree=sh_degree)
        base = {k: v.cpu().numpy().copy() for k, v in r.backward(dL, **kw).items()}
        runs = [{k: v.cpu().numpy().copy() for k, v in r.backward(dL, camera=True, **kw).items()} for _ in range(2)]
        assert set(runs[0]) == set(base) | set(CAM_KEYS)
        for k in base:
            assert np.array_equal(_bits(runs[0][k]), _bits(base[k])), (semantics, k)
        for k in runs[0]:
            assert np.array_equal(_bits(runs[1][k]), _bits(runs[0][k])), (semantics, k)
        assert np.abs(_cam(runs[0])).max() > 0
        grads = r.backward(dL, **kw)
        once = {k: v.clone() for k, v in r.camera_backward(grads, semantics=semantics, sh_degree=sh_degree,
                                                           depth="inverse").items()}
        again = r.camera_backward(grads, semantics=semantics, sh_degree=sh_degree, depth="inverse")
        for k in CAM_KEYS:
            assert torch.equal(once[k].view(torch.int32), again[k].view(torch.int32)), (semantics, k)
            assert np.array_equal(_bits(once[k].cpu().numpy()), _bits(runs[0][k])), (semantics, k)


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_camera_grad_of_four_bands_adds_up_to_the_frame(semantics):
    """Four emulated tile-row bands (forward and backward confined to their rows): the bands' camera gradients add up to
    the whole frame's within 1e-5 M_k."""
    r, scene, cam, bg = _setup()
    inria = semantics == "inria"
    sh_degree = 3 if inria else 0
    kw = dict(semantics=semantics, sh_degree=sh_degree)
    dL, gd = _grads(cam)
    r.draw(cam, plan="sort", tile_history=False, **kw)
    whole = r.backward(dL, dL_ddepth=gd, depth=True, camera=True, **kw)
    got = _cam(whole)
    _, M = _reference(r, cam, whole, semantics, True, sh_degree)
    rows = (cam.height + 15) // 16
    bands = [(0, 1), (1, 2), (2, 4), (4, rows)]
    total = np.zeros(35)
    for b in bands:
        r.draw(cam, plan="sort", tile_history=False, tile_rows=b, **kw)
        part = _cam(r.backward(dL, dL_ddepth=gd, depth=True, camera=True, tile_rows=b, **kw))
        assert np.abs(part).max() > 0, b
        total += part
    _assert_close(total, got.astype(np.float64), M, f"{semantics}: bands", rtol=1e-5)


def test_camera_grad_of_a_frame_without_instances_is_exact_zeros():
    """A camera facing away (R == 0): outputs filled with NaN beforehand come back as exact zeros."""
    import torch
    from gsrast_amd import camera
    r, scene, cam, bg = _setup()
    dL, gd = _grads(cam)
    away = camera.default_camera(cam.width, cam.height, near=0.05, far=50.0, position=(0.0, 0.0, 5.0))
    for semantics in ("gscuda", "inria"):
        r.draw(cam, semantics=semantics, sh_degree=3)
        out = r.backward(dL, camera=True, semantics=semantics, sh_degree=3)
        assert np.abs(_cam(out)).max() > 0
        for k in CAM_KEYS:
            out[k].fill_(float("nan"))
        r.draw(away, semantics=semantics, sh_degree=3)
        assert r.last_num_rendered == 0
        out = r.backward(dL, dL_ddepth=gd, camera=True, semantics=semantics, sh_degree=3)
        for k in CAM_KEYS:
            assert torch.equal(out[k].view(torch.int32), torch.zeros_like(out[k]).view(torch.int32)), (semantics, k)


def test_camera_grad_with_gaussians_behind_the_camera_is_finite():
    """A camera inside the scene: many Gaussians lie behind it (t.z <= 0, culled); the result is finite and matches the
    reference."""
    from gsrast_amd import camera
    from test_depth_cpu import depth_values_f32
    r, scene, cam, bg = _setup()
    inside = camera.default_camera(cam.width, cam.height, near=0.05, far=50.0, position=(0.0, 0.0, 0.0))
    z = depth_values_f32(scene["means3D"], np.asarray(inside.view, np.float32))
    assert (z <= 0).sum() > 100 and (z > 0.2).sum() > 100
    dL, gd = _grads(inside)
    for semantics, sh_degree in (("gscuda", 0), ("inria", 3)):
        r.draw(inside, semantics=semantics, sh_degree=sh_degree, tile_history=False)
        out = r.backward(dL, dL_ddepth=gd, depth="inverse", camera=True, semantics=semantics, sh_degree=sh_degree)
        got = _cam(out)
        assert np.abs(got).max() > 0
        exp, M = _reference(r, inside, out, semantics, "inverse", sh_degree)
        _assert_close(got, exp, M, f"{semantics}: camera inside the scene")


def test_camera_grad_full_size():
    """The 5.8 M-splat bench scene at 1920 x 1080 with a depth gradient: finite, the same bits from two camera passes over
    the same arrays, and within 1e-6 M_k of the float64 reference computed on the device."""
    import torch
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    scene = scenes.garden_like_scene(5_834_784, seed=43)
    span = float(np.max(scene["means3D"][:, :3].max(0) - scene["means3D"][:, :3].min(0)))
    cam = camera.default_camera(1920, 1080, near=0.001 * span, far=span)
    r = SplatRasterizer(1920, 1080)
    r.configure_from_scene(scene)
    del scene
    r.draw(cam)
    dL = torch.randn((3, 1080, 1920), generator=torch.Generator().manual_seed(7)).cuda()
    gd = torch.randn((1080, 1920), generator=torch.Generator().manual_seed(3)).cuda()
    out = r.backward(dL, dL_ddepth=gd, camera=True)
    first = _cam(out)
    second = _cam(r.camera_backward(out, depth=True))
    assert np.isfinite(first).all() and np.abs(first).max() > 0
    assert np.array_equal(_bits(first), _bits(second))
    exp, M = _reference(r, cam, out, "gscuda", True, 0, device=r.device)
    _assert_close(first, exp, M, "full size")


# ---- the camera pass at its loop edges: gsr_camera_backward alone on synthetic per-Gaussian arrays -----------------------
# camera_pass_kernel: a fixed grid of at most 768 x 256 threads, two Gaussians deep in flight (cur, nxt, r_after);
# camera_sum_kernel: rows t, t + 256, ... Up to N = 65 536 the sum loop runs once, up to 196 608 the pass loop runs once, and
# only beyond 393 216 does a thread reach a third iteration, where the radius loaded two iterations ahead is consumed.
LOOP_EDGE_SIZES = [65_537, 196_609, 393_217 + 255]


def _loop_edge_inputs(n, seed):
    """Per-Gaussian arrays of n Gaussians in front of pose P1 (some beyond the +-1.3 tan(fov) clamp), PSD cov3D, random
    gradients, shs and clamp flags; about half of the rows visible, whole waves culled in every iteration of the pass loop,
    the last row visible. Every array of a culled row holds NaN (clamp flags: 255): a culled Gaussian loads nothing but its
    radius."""
    from helpers import posed_camera, world_from_view
    cam = posed_camera(96, 64, eye=(2.0, -1.2, -4.2), target=(0.0, 0.0, 0.0), roll=0.4)
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 6.0, n)
    t = np.stack([rng.uniform(-1.5, 1.5, n) * cam.tan_fovx * z, rng.uniform(-1.5, 1.5, n) * cam.tan_fovy * z, z], 1)
    means = np.ones((n, 4), np.float32)
    means[:, :3] = world_from_view(cam, t)
    A = rng.normal(size=(n, 3, 3)) * 0.1
    S = A @ A.transpose(0, 2, 1)
    a = {"means3D": means,
         "cov3D": np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).astype(np.float32),
         "dL_dmean2D": rng.normal(size=(n, 2)).astype(np.float32),
         "dL_dcov2D": np.concatenate([rng.normal(size=(n, 3)), np.zeros((n, 1))], 1).astype(np.float32),
         "dL_ddepths": rng.normal(size=n).astype(np.float32),
         "dL_dcolors": rng.normal(size=(n, 3)).astype(np.float32),
         "shs": rng.normal(0, 0.35, (n, 48)).astype(np.float32)}
    clamped = rng.uniform(size=(n, 3)) < 0.2
    radii = np.where(rng.uniform(size=n) < 0.5, rng.integers(1, 9, n), 0).astype(np.int32)
    stride = 768 * 256
    for first in (128, 4096, stride + 64, stride + 32768, 2 * stride + 192):          # whole waves, in each iteration
        if first + 64 <= n:
            radii[first:first + 64] = 0
    radii[-1] = 3
    off = radii <= 0
    for v in a.values():
        v[off] = np.nan
    flags = clamped.astype(np.uint8)
    flags[off] = 255
    return cam, a, radii, clamped, flags


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
@pytest.mark.parametrize("n", LOOP_EDGE_SIZES)
def test_camera_pass_at_its_loop_edges(n, semantics):
    """gsr_camera_backward on synthetic arrays at the sizes where the sum loop takes a second turn, the pass loop a second
    and a third — in both instantiations (upstream: SH colour of degree 3, with an inverse-depth gradient). Finite although
    the culled rows hold NaN; within 1e-6 M_k of the float64 reference computed on the device; the same bits twice."""
    import torch
    from gsrast_amd import _capi
    inria = semantics == "inria"
    cam, a, radii, clamped, flags = _loop_edge_inputs(n, seed=n % 1000)
    off = radii <= 0
    assert 0.4 * n < (~off).sum() < 0.6 * n and radii[-1] > 0
    assert all(np.isnan(v[off]).all() for v in a.values())
    dev = torch.device("cuda:0")
    d = {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
    rad, flg = torch.from_numpy(radii).to(dev), torch.from_numpy(flags).to(dev)
    view, proj, pos = (torch.from_numpy(np.asarray(v, np.float32).copy()).to(dev) for v in (cam.view, cam.proj, cam.cam_pos))
    L = _capi.lib()
    scratch = torch.empty(int(L.gsr_camera_backward_scratch_bytes(n)), dtype=torch.uint8, device=dev)
    outs = []
    for _ in range(2):
        out = torch.full((35,), float("nan"), dtype=torch.float32, device=dev)
        scratch.fill_(255)
        args = _capi.CameraBackwardArgs()
        args.struct_size = C.sizeof(_capi.CameraBackwardArgs)
        args.flags = (_capi.GSR_FLAG_SEMANTICS_INRIA | _capi.GSR_FLAG_DEPTH_INVERSE) if inria else 0
        args.num_gaussians, args.width, args.height = n, cam.width, cam.height
        args.means3D, args.view_matrix, args.proj_matrix, args.cam_pos = (t.data_ptr() for t in (d["means3D"], view, proj, pos))
        args.tan_fovx, args.tan_fovy = cam.tan_fovx, cam.tan_fovy
        args.cov3D, args.radii = d["cov3D"].data_ptr(), rad.data_ptr()
        if inria:
            args.shs, args.clamped, args.sh_dims = d["shs"].data_ptr(), flg.data_ptr(), 3
            args.dL_dcolors = d["dL_dcolors"].data_ptr()
        args.dL_dmean2D, args.dL_dcov2D, args.dL_ddepths = (d[k].data_ptr() for k in ("dL_dmean2D", "dL_dcov2D", "dL_ddepths"))
        args.dL_dview_matrix, args.dL_dproj_matrix, args.dL_dcam_pos = out[0:16].data_ptr(), out[16:32].data_ptr(), out[32:35].data_ptr()
        args.scratch = scratch.data_ptr()
        args.stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _capi.check(L.gsr_camera_backward(C.byref(args)), "gsr_camera_backward")
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
    got = outs[0]
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    exp, M = camera_grad(d["means3D"], cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, rad,
                         d["cov3D"], d["dL_dmean2D"], d["dL_dcov2D"], dL_ddepths=d["dL_ddepths"], inverse=inria, inria=inria,
                         shs=d["shs"] if inria else None, sh_degree=3, dL_dcolors=d["dL_dcolors"] if inria else None,
                         clamped=torch.from_numpy(clamped).to(dev) if inria else None, device=dev)
    _assert_close(got, exp, M, f"{semantics}, n = {n}")
    assert M[:16].max() > 0 and M[16:32].max() > 0
    assert (M[32:] > 0).all() if inria else (got[32:] == 0).all()
