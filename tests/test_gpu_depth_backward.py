"""GPU: gsr_backward with the depth channel (dL_dout_depth). The reference is the superposition of two float64 blend backwards
(oracle/backward_np.py): the colour one, and one of colours (d_i, 0, 0) against (dL_ddepth, 0, 0) over a zero background;
dL_ddepths is the latter's colour gradient, and dL_dmeans3D is the chain of the summed 2-D gradients plus the view-row term."""
import numpy as np
import pytest

from test_depth_cpu import depth_mean_term, depth_values_f32

pytestmark = pytest.mark.gpu

RTOL = 2e-4       # as tests/test_gpu_backward.py: float32 sums in some order against float64


def _close(got, exp, what, rtol=RTOL):
    scale = max(1e-6, float(np.abs(exp).max()))
    err = float(np.abs(np.asarray(got, np.float64) - exp).max())
    assert err <= rtol * scale, f"{what}: max abs err {err} at scale {scale}"


def _setup(seed=2, w=100, h=70, n=1200, bg=(0.2, 0.5, 0.9)):
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    scene = scenes.garden_like_scene(n, seed=seed)
    scene["means3D"][:, :3] *= 0.25
    cam = camera.default_camera(w, h, near=0.05, far=50.0)
    r = SplatRasterizer(w, h, background=bg)
    r.configure_from_scene(scene)
    return r, scene, cam, bg


CASES = [("gscuda", True, "sorted", True), ("gscuda", "inverse", "sorted", True), ("gscuda", True, "sorted", False),
         ("gscuda", True, "block_lists", True), ("gscuda", "inverse", "block_lists", False),
         ("inria", True, "sorted", True), ("inria", "inverse", "sorted", False)]


@pytest.mark.parametrize("semantics,mode,feed,wide", CASES)
def test_depth_backward_matches_the_float64_superposition(semantics, mode, feed, wide):
    import torch
    from oracle import backward_np as B
    from helpers import check_backward_chain, check_backward_chain_inria
    r, scene, cam, bg = _setup()
    w, h = cam.width, cam.height
    inria = semantics == "inria"
    kw = dict(semantics=semantics, sh_degree=0, tile_history=False)
    # the forward: the sorted lists, then (block_lists) a call that leaves them unwritten and hands the block lists to the
    # backward; neither writes out_depth (the backward recomputes d_i: any receipt serves)
    r.draw(cam, plan="sort" if feed == "sorted" else "blocks", **kw)
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    plist = r.map_binning_state()["values"].cpu().numpy().view(np.uint32).astype(np.int64)
    if feed == "block_lists":
        r.draw(cam, plan="blocks", sorted_lists=False, **kw)
        assert not r.last_lists_written
    rng = np.random.default_rng(11)
    dL = rng.normal(size=(3, h, w)).astype(np.float32)
    gd = rng.normal(size=(h, w)).astype(np.float32)
    got = {k: v.cpu().numpy().copy() for k, v in
           r.backward(torch.from_numpy(dL), dL_ddepth=torch.from_numpy(gd), depth=mode, wide_sums=wide, semantics=semantics,
                      sh_degree=0).items()}
    assert "dL_ddepths" in got

    inverse = mode == "inverse"
    ranges = im["ranges"].view(np.uint32).astype(np.int64)
    out64, ft64, nc64 = B.blend_forward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, w, h, bg,
                                        t_cutoff=1e-4 if inria else 0.001)
    assert (nc64 != im["nContrib"].view(np.uint32)).sum() <= 2
    exp_c = B.blend_backward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, nc64, ft64, w, h, bg, dL)
    d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), inverse).astype(np.float64)
    g3 = np.zeros((3, h, w))
    g3[0] = gd
    exp_d = B.blend_backward(g["means2D"], g["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), ranges, plist, nc64, ft64, w, h,
                             (0.0, 0.0, 0.0), g3)
    what = f"{semantics}/{mode}/{feed}/wide={wide}"
    _close(got["dL_ddepths"], exp_d["dL_dcolor"][:, 0], f"{what}: dL_ddepths")
    _close(got["dL_dcolors"], exp_c["dL_dcolor"], f"{what}: dL_dcolors")
    _close(got["dL_dmean2D"], exp_c["dL_dmean2D"] + exp_d["dL_dmean2D"], f"{what}: dL_dmean2D")
    _close(got["dL_dconic_opacity"][:, :3], exp_c["dL_dconic"] + exp_d["dL_dconic"], f"{what}: dL_dconic")
    _close(got["dL_dconic_opacity"][:, 3], exp_c["dL_dopacity"] + exp_d["dL_dopacity"], f"{what}: dL_dopacity")
    assert np.abs(exp_d["dL_dcolor"][:, 0]).max() > 0 and np.abs(exp_d["dL_dmean2D"]).max() > 0
    # the chain: what the summed 2-D gradients give, plus dL_ddepths (V[2], V[6], V[10]) (-1 / z^2 for inverse depth)
    vis = np.nonzero(g["radii"] > 0)[0]
    term = depth_mean_term(scene["means3D"][:, :3], np.asarray(cam.view, np.float32), got["dL_ddepths"], inverse)
    assert (got["dL_ddepths"][g["radii"] <= 0] == 0).all()
    chain = dict(got)
    chain["dL_dmeans3D"] = got["dL_dmeans3D"].copy()
    chain["dL_dmeans3D"][:, :3] -= term
    if inria:
        clamped = r.geom.view(_clamped_ptr(r), 3 * r.num_gaussians, torch.uint8).cpu().numpy().reshape(-1, 3)
        check_backward_chain_inria(chain, g, scene, cam, w, h, vis, 0, clamped)
    else:
        check_backward_chain(chain, g, scene, cam, w, h, vis)
    assert float(np.abs(term[vis]).max()) > 1e-3 * float(np.abs(got["dL_dmeans3D"][vis, :3]).max())


def _clamped_ptr(r):
    import ctypes as C
    from gsrast_amd import _capi
    st = _capi.GeometryState()
    r.lib.gsr_geometry_from_chunk(r.geom.base(), r.num_gaussians, C.byref(st))
    return st.clamped


@pytest.mark.parametrize("wide", [True, False])
def test_backward_without_depth_is_unchanged_by_a_depth_forward(wide):
    """Every output of a backward without dL_ddepth is the same whether the forward call wrote out_depth or not."""
    import torch
    r, scene, cam, bg = _setup(seed=3)
    dL = torch.from_numpy(np.random.default_rng(4).normal(size=(3, cam.height, cam.width)).astype(np.float32))
    r.draw(cam, tile_history=False)
    a = {k: v.cpu().numpy().copy() for k, v in r.backward(dL, wide_sums=wide).items()}
    r.draw(cam, tile_history=False, depth=True)
    b = {k: v.cpu().numpy().copy() for k, v in r.backward(dL, wide_sums=wide, dL_ddepth=None).items()}
    assert sorted(a) == sorted(b) and "dL_ddepths" not in b
    for k in a:       # (float atomics, or double ones rounded once: run-to-run noise only)
        _close(b[k], a[k].astype(np.float64), k, rtol=1e-6 if wide else 1e-5)


def test_depth_sums_are_reproducible_and_left_zero():
    import torch
    r, scene, cam, bg = _setup(seed=5, w=128, h=96, n=4000)
    rng = np.random.default_rng(6)
    dL = torch.from_numpy(rng.normal(size=(3, cam.height, cam.width)).astype(np.float32))
    gd = torch.from_numpy(rng.normal(size=(cam.height, cam.width)).astype(np.float32))
    # (sorted lists: every sum in double; the block lists' per-entry sums are floats first, added in some order)
    for kw, exact in ((dict(plan="sort"), True), (dict(plan="blocks", sorted_lists=False), False)):
        r.draw(cam, tile_history=False, **kw)
        runs = [{k: v.cpu().numpy().copy() for k, v in r.backward(dL, dL_ddepth=gd, depth="inverse").items()} for _ in range(3)]
        assert float(np.abs(runs[0]["dL_ddepths"]).max()) > 0
        for run in runs[1:]:
            for k in ("dL_ddepths", "dL_dmeans3D", "dL_dmean2D"):
                if exact:
                    assert np.array_equal(run[k], runs[0][k]), (kw, k)
                else:
                    _close(run[k], runs[0][k].astype(np.float64), f"{kw} {k}", rtol=1e-5)
        assert bool((r._bw.scratch["depth_sums_f64"] == 0).all()) and bool((r._bw.scratch["sums_f64"] == 0).all())
