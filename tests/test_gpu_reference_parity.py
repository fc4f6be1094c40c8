"""GPU: gsr_forward against the reference itself — the reference's own CUDA files compiled for the host
(oracle/_ref/libgscuda_ref.so, oracle/ref_cpu.py) — with no oracle between. The library travels with the working tree; the
reference tree is never read here. The rule is the one tests/test_gpu_parity.py applies against the oracle: every integer and
per-Gaussian output, both lists, the ranges, finalT and nContrib bit for bit, pixels within helpers.PIXEL_TOL (2e-6).
Every frame runs under both binning plans; the dense frame is the one the block plan feeds the blend from its block lists.
(What a host build of the reference does and does not pin: tests/test_reference_pin.py.)"""
import functools

import numpy as np
import pytest

import reference_frames as F
from helpers import assert_blend_parity
from oracle import ref_cpu

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref_cpu.available(), reason="neither oracle/_ref/libgscuda_ref.so nor a reference tree to build it from")]

PLAN = "auto"


@pytest.fixture(autouse=True, params=["sort", "blocks"])
def binning_plan(request):
    global PLAN
    PLAN = request.param
    yield
    PLAN = "auto"


FRAMES = {
    "config1": lambda: F.golden(True),
    "radius_path": lambda: F.golden(False),
    "anisotropic": lambda: F.anisotropic(200, 120, 3000, 7),
    "equal_keys": F.equal_keys,
    "opaque_stack": F.opaque_stack,
    "single_instance": F.single_instance,
    "extreme_in_range": lambda: F.extreme_but_finite(7, **F.EXTREME_BOUNDED),      # (extents up to 1.1e9: the family's largest)
    "wide_grid": F.wide_grid,
    "wide_grid_all_columns": F.wide_grid_all_columns,
    "dense": F.dense,
}


@functools.lru_cache(maxsize=None)
def _reference(name):
    scene, cam, bg, kw = FRAMES[name]()
    ref = ref_cpu.forward(scene, cam, bg, **kw)
    assert F.conversions_in_range(ref, cam).all(), name
    return scene, cam, bg, kw, ref


def _run(scene, cam, bg, use_rects=True, **kw):
    """As test_gpu_parity._run: a first draw, every chunk zeroed (what a call leaves unwritten then compares equal to the
    reference's zero-filled chunks), and the draw that is compared."""
    import torch
    from gsrast_amd.rasterizer import SplatRasterizer
    assert torch.cuda.is_available(), "no HIP device"
    r = SplatRasterizer(cam.width, cam.height, background=bg)
    r.configure_from_scene(scene, use_rects=use_rects)
    r.draw(cam, plan=PLAN, **kw)
    for cb in (r.geom, r.image, r.binning):
        if cb.tensor is not None:
            cb.tensor.zero_()
    if r.rects is not None:
        r.rects.zero_()
    r.out_color.zero_()
    img = r.draw(cam, plan=PLAN, **kw).cpu().numpy().copy()
    return r, img


def _compare(r, img, ref, what):
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    assert np.array_equal(g["radii"], ref["radii"]), what
    assert np.array_equal(g["tilesTouched"].view(np.uint32), ref["tilesTouched"]), what
    assert np.array_equal(g["pointOffsets"].view(np.uint32), ref["pointOffsets"]), what
    if ref["rects"] is not None:
        assert np.array_equal(r.rects.cpu().numpy(), ref["rects"]), what
    for k in ("means2D", "depths", "cov3D", "rgb", "conicOpacity"):
        assert np.array_equal(g[k].view(np.uint32), ref[k].view(np.uint32)), (what, k)
    R = ref["num_rendered"]
    assert r.last_num_rendered == R, (what, r.last_num_rendered, R)
    b = {k: v.cpu().numpy() for k, v in r.map_binning_state().items()}
    if r.last_plan != "blocks":
        # (the library emits the pairs in another order than the reference's index order: the same multiset — test_gpu_parity._compare_all;
        # the block plan keeps its block lists there)
        ku, vu = b["keys_unsorted"].view(np.uint64), b["values_unsorted"].view(np.uint32)
        o_g, o_e = np.lexsort((vu, ku)), np.lexsort((ref["values_unsorted"], ref["keys_unsorted"]))
        assert np.array_equal(ku[o_g], ref["keys_unsorted"][o_e]) and np.array_equal(vu[o_g], ref["values_unsorted"][o_e]), what
    assert np.array_equal(b["keys"].view(np.uint64), ref["keys"]), what
    assert np.array_equal(b["values"].view(np.uint32), ref["values"]), what
    im = {k: v.cpu().numpy() for k, v in r.map_image_state().items()}
    assert np.array_equal(im["ranges"].view(np.uint32), ref["ranges"]), what
    assert_blend_parity(img, im["finalT"], im["nContrib"], ref, what, bitwise_t=True)


@pytest.mark.parametrize("name", list(FRAMES))
def test_forward_against_the_reference_itself(name):
    scene, cam, bg, kw, ref = _reference(name)
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    r, img = _run(scene, cam, bg, **kw)
    what = f"{name} {cam.width}x{cam.height} N={scene['means3D'].shape[0]} R={ref['num_rendered']} plan={r.last_plan}"
    assert ref["num_rendered"] >= 1, what
    if ref["num_rendered"] > 1:
        assert r.last_plan == ("generic" if (gx > 255 or gy > 255) else PLAN), what
    _compare(r, img, ref, what)
    if name == "single_instance":
        assert ref["num_rendered"] == 1 and np.array_equal(img, ref["out_color"]) and not ref["ranges"].any()
    if name == "dense":
        visible = int((ref["tilesTouched"] > 0).sum())
        assert ref["num_rendered"] >= 48 * visible > 0, (ref["num_rendered"], visible)
        if PLAN == "blocks":
            assert not r.last_blend_from_lists, "the dense frame is meant to be block-fed"
    if name == "wide_grid_all_columns":
        assert int(((ref["keys"] >> np.uint64(32)) % np.uint64(gx)).max()) == 256


def test_nothing_rendered_against_the_reference_itself():
    """R == 0: the reference returns before the binning allocator and leaves out_color as it was (GSCuda.cu:775-778); so does
    gsr_forward, with the same per-Gaussian outputs."""
    import torch
    from gsrast_amd.rasterizer import SplatRasterizer
    scene, cam, bg, kw = F.nothing_visible()
    ref = ref_cpu.forward(scene, cam, bg, **kw)
    assert ref["num_rendered"] == 0 and ref["alloc_calls"] == (1, 1, 0) and (ref["out_color"] == 0.25).all()
    assert torch.cuda.is_available(), "no HIP device"
    r = SplatRasterizer(cam.width, cam.height, background=bg)
    r.configure_from_scene(scene)
    r.out_color.fill_(0.25)
    r.draw(cam, plan=PLAN)
    assert r.last_num_rendered == 0 and len(r.binning.calls) == 0
    assert np.array_equal(r.out_color.cpu().numpy(), ref["out_color"])
    g = {k: v.cpu().numpy() for k, v in r.map_geometry_state().items()}
    assert np.array_equal(g["radii"], ref["radii"]) and np.array_equal(g["tilesTouched"].view(np.uint32), ref["tilesTouched"])
    assert np.array_equal(g["pointOffsets"].view(np.uint32), ref["pointOffsets"])
