"""GPU: the forward depth channel (gsr_forward_args.out_depth). Non-interference — a call with out_depth changes nothing else
it writes, in any blend variant —, bit-exactness against the colour channel of a call with colors_precomp = (d, d, d) over a
zero background, the float64 blend on the golden scene, and the edges: R == 0, row bands, lists walked to their end."""
import numpy as np
import pytest

from test_depth_cpu import depth_values_f32

pytestmark = pytest.mark.gpu

W, H = 160, 112


def _scenes():
    from gsrast_amd import camera, scenes
    from helpers import load_golden
    g_scene, g_cam, g_bg, _ = load_golden()
    return [("golden", g_scene, g_cam, g_bg),
            ("isotropic", scenes.isotropic_scene(3000, 42), camera.default_camera(W, H, near=0.05, far=50.0), (0.1, 0.2, 0.3)),
            ("garden", scenes.garden_like_scene(40_000, seed=43), camera.default_camera(W, H, near=0.05, far=80.0), (0.0, 0.0, 0.0)),
            ("far", scenes.garden_like_scene(40_000, seed=43),
             camera.default_camera(W, H, near=0.05, far=100.0, position=(0.0, 0.0, -30.0)), (0.3, 0.3, 0.3))]


# every forced blend variant (tile_history=False throughout: the call's choice depends on nothing but its own inputs)
VARIANTS = [("sort", dict(plan="sort", deep_tiles=False)),
            ("blocks", dict(plan="blocks", overlap_emit=False)),
            ("blocks_overlap", dict(plan="blocks", overlap_emit=True)),
            ("block_lists", dict(plan="blocks", sorted_lists=False, overlap_emit=False)),
            ("deep_all", dict(plan="sort", deep_tiles="all")),
            ("deep_all8", dict(plan="sort", deep_tiles="all8")),
            ("deep_all16", dict(plan="sort", deep_tiles="all16")),
            ("inria", dict(plan="sort", deep_tiles=False, semantics="inria", sh_degree=0)),
            ("inria_blocks", dict(plan="blocks", overlap_emit=False, semantics="inria", sh_degree=0))]


def _rast(scene, cam, bg):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, background=bg)
    r.configure_from_scene(scene)
    return r


def _state(r):
    im = r.map_image_state()
    return (r.out_color.cpu().numpy().copy(), im["finalT"].cpu().numpy().copy(), im["nContrib"].cpu().numpy().copy(),
            r.last_num_rendered, int(r.last_receipt.plan_used))


def _same_bits(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))


def _depth_colors(r, cam, inverse):
    import torch
    d = depth_values_f32(r.means3D.cpu().numpy(), np.asarray(cam.view, np.float32), inverse)
    return torch.from_numpy(np.repeat(d[:, None], 3, 1).copy()).to(r.device)


@pytest.mark.parametrize("variant", [v[0] for v in VARIANTS])
def test_depth_changes_nothing_else_and_is_a_colour_channel(variant):
    kw = dict(VARIANTS)[variant]
    for name, scene, cam, bg in _scenes():
        r = _rast(scene, cam, bg)
        ref = _rast(scene, cam, (0.0, 0.0, 0.0))
        r.draw(cam, tile_history=False, **kw)
        base = _state(r)
        assert base[3] > 0, name
        for mode in (True, "inverse"):
            r.out_depth = None
            r.draw(cam, tile_history=False, depth=mode, **kw)
            got = _state(r)
            what = f"{name}/{variant}/{mode}"
            for i, k in enumerate(("out_color", "finalT", "nContrib")):
                _same_bits(got[i], base[i], f"{what}: {k}")
            assert got[3:] == base[3:], (what, got[3:], base[3:])
            depth = r.out_depth.cpu().numpy().copy()
            assert np.isfinite(depth).all(), what
            # the same variant, colours (d, d, d), zero background: channel 0 is the depth channel, bit for bit
            ref.draw(cam, tile_history=False, colors_precomp=_depth_colors(r, cam, mode == "inverse"), **kw)
            assert ref.last_num_rendered == base[3], what
            _same_bits(depth, ref.out_color[0].cpu().numpy(), f"{what}: out_depth against colour channel 0")
            assert float(np.abs(depth).max()) > 0, what


def test_depth_keeps_the_staged_record_count():
    for name, scene, cam, bg in _scenes()[:3]:
        r = _rast(scene, cam, bg)
        for kw in (dict(plan="sort"), dict(plan="blocks"), dict(plan="sort", deep_tiles="all")):
            r.draw(cam, tile_history=False, count_staged=True, **kw)
            base = (r.last_records_staged, _state(r))
            r.draw(cam, tile_history=False, count_staged=True, depth=True, **kw)
            assert r.last_records_staged == base[0] > 0, (name, kw)
            _same_bits(_state(r)[0], base[1][0], f"{name} {kw}")


@pytest.mark.parametrize("inverse", [False, True])
def test_depth_against_the_float64_blend(inverse):
    from oracle import backward_np as B
    from helpers import PIXEL_TOL, load_golden
    scene, cam, bg, _ = load_golden()
    r = _rast(scene, cam, bg)
    r.draw(cam, depth="inverse" if inverse else True, tile_history=False)
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    plist = r.map_binning_state()["values"].cpu().numpy().view(np.uint32).astype(np.int64)
    d = depth_values_f32(scene["means3D"], np.asarray(cam.view, np.float32), inverse).astype(np.float64)
    out, ft, nc = B.blend_forward(g["means2D"], g["conicOpacity"], np.repeat(d[:, None], 3, 1),
                                  im["ranges"].view(np.uint32).astype(np.int64), plist, cam.width, cam.height, (0.0, 0.0, 0.0))
    assert (nc != im["nContrib"].view(np.uint32)).sum() == 0
    err = float(np.abs(out[0] - r.out_depth.cpu().numpy()).max())
    scale = max(1.0, float(np.abs(d).max()))
    print(f"[depth] golden, inverse={inverse}: max abs err {err:.3e} at depth scale {scale:.3f}")
    assert err <= PIXEL_TOL * scale
    assert np.allclose(r.opacity_map().cpu().numpy(), 1.0 - ft, atol=1e-6)


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_depth_of_a_frame_without_instances_is_zero(semantics):
    import torch
    from gsrast_amd import camera, scenes
    scene = scenes.isotropic_scene(500, 7)
    away = camera.default_camera(W, H, near=0.05, far=50.0, position=(0.0, 0.0, 5.0))     # the scene is behind this camera
    r = _rast(scene, away, (0.2, 0.2, 0.2))
    r.out_depth = torch.full((H, W), float("nan"), device=r.device)
    r.draw(away, depth=True, semantics=semantics, sh_degree=0)
    assert r.last_num_rendered == 0
    assert bool((r.out_depth == 0).all())


@pytest.mark.parametrize("kw", [dict(plan="sort"), dict(plan="blocks", overlap_emit=False)])
def test_depth_of_row_bands(kw):
    import torch
    from gsrast_amd import camera, scenes
    scene = scenes.garden_like_scene(40_000, seed=43)
    cam = camera.default_camera(W, H, near=0.05, far=80.0)
    r = _rast(scene, cam, (0.0, 0.0, 0.0))
    r.draw(cam, depth=True, tile_history=False, **kw)
    whole = r.out_depth.cpu().numpy().copy()
    gy = (H + 15) // 16
    stitched = np.full((H, W), np.nan, np.float32)
    for b0, b1 in ((0, 2), (2, 5), (5, gy)):
        r.out_depth = torch.full((H, W), float("nan"), device=r.device)
        r.draw(cam, depth=True, tile_history=False, tile_rows=(b0, b1), **kw)
        band = r.out_depth.cpu().numpy()
        y0, y1 = 16 * b0, min(H, 16 * b1)
        assert np.isfinite(band[y0:y1]).all(), (b0, b1)
        assert np.isnan(band[:y0]).all() and np.isnan(band[y1:]).all(), (b0, b1)
        stitched[y0:y1] = band[y0:y1]
    _same_bits(stitched, whole, "bands stitched against the whole frame")


def test_depth_of_faint_splats_walks_every_list_to_its_end():
    from gsrast_amd import camera, scenes
    scene = scenes.isotropic_scene(4000, 11)
    scene["opacities"] = np.full_like(scene["opacities"], 0.008)        # (alpha <= 0.008: just above the 1/255 cut)
    cam = camera.default_camera(W, H, near=0.05, far=50.0)
    r = _rast(scene, cam, (0.0, 0.0, 0.0))
    ref = _rast(scene, cam, (0.0, 0.0, 0.0))
    for kw in (dict(plan="sort", deep_tiles=False), dict(plan="sort", deep_tiles="all"), dict(plan="blocks", overlap_emit=False)):
        r.draw(cam, depth=True, tile_history=False, **kw)
        ft = r.map_image_state()["finalT"].cpu().numpy()
        assert ft.min() > 0.01, "no pixel may saturate: every list is walked to its end"
        ref.draw(cam, tile_history=False, colors_precomp=_depth_colors(r, cam, False), **kw)
        _same_bits(r.out_depth.cpu().numpy(), ref.out_color[0].cpu().numpy(), f"faint {kw}")
        assert float(r.out_depth.max()) > 0
