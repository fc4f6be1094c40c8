"""GPU: the absolute screen-space gradient, gsr_absgrad (include/gsrast_amd_absgrad.h; SplatRasterizer.absgrad,
autograd.FrameSlot(absgrad=True), densify.DensityStats.update(absgrad=True)). The reference is tests/absgrad_ref.py's float64
walk over the forward state read back from the GPU; tests/test_absgrad_cpu.py pins it to the project's oracle and establishes
that the scenes used here tell sum-of-abs from abs-of-sum and the joint result from the parts' sum.

Acceptance, per Gaussian and component, is the render backward's rule of tests/helpers.py, unchanged:
    |got - A| <= BW_TAU (k + BW_C) M + BW_ATOL, and a row nothing blended is +0.0 bit for bit.
Worst |err| / ((k + BW_C) M) measured on one MI355X (the bound allows BW_TAU = 1.1e-7; profiles/absgrad_cost.txt has every case):
one tile 1.8e-9 (length 1) to 1.05e-8 (length 256, faint); edge tiles 4.3e-9 (gscuda) and 4.8e-9 (inria), the same for both
plans; colour + depth 9.6e-9, + inverse depth 4.3e-9, + alpha 6.5e-9, all three 8.4e-9; the clamp scene 2.7e-9 to 4.5e-9; one
splat over 64 tiles 5.0e-9, its bands 3.3e-9 to 5.0e-9; through autograd (colour + depth) 8.8e-9 and 9.6e-9."""
import numpy as np
import pytest

import absgrad_ref as R
from helpers import BW_C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0


def _rasterizer(scene, cam):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, device=DEV, background=R.BACKGROUND)
    r.configure_from_scene(scene)
    return r


def _state(r):
    """The forward state of r's last draw(), as numpy arrays under the oracle's names."""
    g, im = r.map_geometry_state(), r.map_image_state()
    return {"means2D": g["means2D"].cpu().numpy(), "conicOpacity": g["conicOpacity"].cpu().numpy(), "rgb": g["rgb"].cpu().numpy(),
            "ranges": im["ranges"].cpu().numpy().view(np.uint32), "nContrib": im["nContrib"].cpu().numpy().view(np.uint32),
            "finalT": im["finalT"].cpu().numpy(),
            "values": (r.map_binning_state()["values"].cpu().numpy().view(np.uint32) if r.last_num_rendered else np.zeros(0, np.uint32))}


def _chunks(r):
    return [t.clone() for t in (r.geom.tensor, r.binning.tensor, r.image.tensor) if t is not None]


def _call(r, cam, terms="colour", semantics="gscuda", tile_rows=None, seed=5):
    """One gsr_absgrad call for r's last draw() into a tensor with a sentinel row on either side. Checks what every call must
    leave: the sentinels, an all-zero scratch, the three chunks byte for byte. -> float32 [N,2] on the host"""
    import torch
    gc, gd, ga = (torch.from_numpy(a).to(DEV) for a in R.pixel_gradients(cam, seed))
    depth = terms in ("colour+depth", "colour+inverse", "all")
    n = r.num_gaussians
    buf = torch.full((n + 2, 2), SENTINEL, dtype=torch.float32, device=DEV)
    before = _chunks(r)
    out = r.absgrad(gc, dL_ddepth=gd if depth else None, depth=("inverse" if terms == "colour+inverse" else True) if depth else None,
                    dL_dalpha=ga if terms in ("colour+alpha", "all") else None, semantics=semantics, tile_rows=tile_rows,
                    into=buf[1:n + 1])
    assert out.data_ptr() == buf[1:].data_ptr()
    host = buf.cpu().numpy()
    assert (host[0] == SENTINEL).all() and (host[n + 1] == SENTINEL).all(), "a write outside the output"
    assert not bool(r._bw.scratch["absgrad_sums_f64"].view(torch.int64).any()), "the scratch is not left zero"
    after = _chunks(r)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "a chunk was written"
    return host[1:n + 1].copy()


def _check(got, ref, what):
    """The bound and the support rule; prints and returns the worst |err| / ((k + BW_C) M)."""
    assert got.dtype == np.float32 and got.shape == ref["A"].shape and np.isfinite(got).all(), what
    none = ref["pixels"] == 0
    assert (got[none].view(np.uint32) == 0).all(), (what, "a row nothing blended must be +0.0 bit for bit")
    assert (got[ref["free_pixels"] == 0].view(np.uint32) == 0).all(), (what, "clamped on every pixel: no share")
    err = np.abs(got.astype(np.float64) - ref["A"])
    scale = (ref["k"].astype(np.float64) + BW_C)[:, None] * ref["M"]
    ratio = np.where(ref["M"] > 0, err / np.maximum(scale, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"[absgrad] {what}: {int((~none).sum())} blended, worst |err| / ((k + {BW_C:g}) M) = {worst:.3e}")
    over = err > R.bound(ref)
    assert not over.any(), (what, f"{int(over.any(1).sum())} Gaussians over the bound; worst ratio {worst:.3e}",
                            np.nonzero(over.any(1))[0][:8])
    assert (got[ref["free_pixels"] > 0] > 0).all(), (what, "a blended, unclamped Gaussian without a share")
    return worst


def _draw_and_check(r, scene, cam, terms="colour", semantics="gscuda", what="", tile_rows=None, **draw):
    r.draw(cam, semantics=semantics, sh_degree=0, tile_rows=tile_rows, **draw)
    st = _state(r)
    ref = R.reference(st, scene, cam, terms, semantics, tile_rows)
    on = ref["n_contrib"] >= 0
    assert np.array_equal(ref["n_contrib"][on], st["nContrib"].astype(np.int64)[on]), (what, "the forward state is not the reference's")
    got = _call(r, cam, terms, semantics, tile_rows)
    _check(got, ref, what or terms)
    return got, ref


# ---- one 16 x 16 tile: the wave's batch of 64 and the round of 256; faint records; an opaque front ---------------------------
@pytest.mark.parametrize("opaque", [False, True], ids=["faint", "opaque"])
@pytest.mark.parametrize("length", R.LIST_LENGTHS)
def test_one_tile_lists_of_every_length(length, opaque):
    import contrib_ref
    scene, cam = contrib_ref.one_tile_scene(length, opaque)
    r = _rasterizer(scene, cam)
    got, ref = _draw_and_check(r, scene, cam, what=f"length {length} {'opaque' if opaque else 'faint'}")
    st = _state(r)
    assert int(st["ranges"][0, 1]) - int(st["ranges"][0, 0]) == length
    if not opaque:
        assert int(st["nContrib"].max()) == length
    elif length >= 255:
        assert (st["nContrib"] < length).sum() >= 100       # pixels that end below the list length
    assert got.sum() > 0


# ---- 40 x 24: partial right and bottom tiles; both semantics, both plans; every combination of terms -------------------------
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_edge_tiles_both_semantics_and_both_plans(semantics):
    import contrib_ref
    scene, cam = contrib_ref.edge_scene()
    r = _rasterizer(scene, cam)
    a, ref = _draw_and_check(r, scene, cam, "colour", semantics, f"edge {semantics} sort", plan="sort")
    assert r.last_plan == "sort"
    b, ref_b = _draw_and_check(r, scene, cam, "colour", semantics, f"edge {semantics} blocks", plan="blocks")
    assert r.last_plan == "blocks" and r.last_lists_written
    assert np.array_equal(ref["A"], ref_b["A"])              # the same lists either way
    assert (ref["pixels"] == 0).sum() >= 4


@pytest.mark.parametrize("terms", R.TERMS)
@pytest.mark.parametrize("name", ["edge", "clamp"])
def test_every_combination_of_terms_against_the_joint_reference(name, terms):
    import contrib_ref
    scene, cam = contrib_ref.edge_scene() if name == "edge" else R.clamp_scene()
    r = _rasterizer(scene, cam)
    got, ref = _draw_and_check(r, scene, cam, terms, what=f"{name} {terms}")
    if name == "clamp":
        partly = (ref["free_pixels"] > 0) & (ref["free_pixels"] < ref["pixels"])
        assert partly.sum() >= 12                            # records with raw > 0.99 on some of their pixels


# ---- 128 x 128: one splat over 64 tiles; bands; beside gsr_backward ----------------------------------------------------------
def test_one_splat_over_64_tiles_bands_and_the_signed_gradient():
    import torch
    import contrib_ref
    from helpers import BW_ATOL, BW_TAU
    scene, cam = contrib_ref.fill_scene()
    r = _rasterizer(scene, cam)
    whole, ref = _draw_and_check(r, scene, cam, what="fill, whole frame")
    assert int(ref["pixels"][0]) > 6400 and whole[0].min() > 0
    # beside the signed sums of the same frame: A >= |dL_dmean2D| less the two bounds (colour only: M is the same sum for both)
    gc = torch.from_numpy(R.pixel_gradients(cam)[0]).to(DEV)
    kw = dict(outputs=("dL_dmean2D", "dL_dconic_opacity"), wide_sums=True)
    signed = r.backward(gc, **kw)["dL_dmean2D"].cpu().numpy().astype(np.float64)
    bound = R.bound(ref)
    assert (np.abs(signed - ref["signed"]) <= bound).all()
    assert (whole >= np.abs(signed) - 2.0 * bound).all()
    far = (whole > 2.0 * np.abs(signed)).any(axis=1)[ref["free_pixels"] > 0]
    assert far.mean() >= 0.3                                 # ... and it is not the absolute value of that sum
    # gsr_backward behind gsr_absgrad: the bits it gives without it
    first = {k: v.clone() for k, v in r.backward(gc, **kw).items()}
    _call(r, cam)
    second = r.backward(gc, **kw)
    assert all(torch.equal(first[k].view(torch.int32), second[k].view(torch.int32)) for k in first)
    # a band: rows 1 and 2 alone, against the reference restricted to them
    band, ref_band = _draw_and_check(r, scene, cam, what="fill, rows 1-2", tile_rows=(1, 3))
    assert 0 < band.sum() < whole.sum()
    # two bands add up to the whole frame: each within its own bound, and (k + c) M of the whole frame covers both
    parts = [_draw_and_check(r, scene, cam, what=f"fill, rows {rows}", tile_rows=rows) for rows in ((0, 3), (3, 8))]
    added = parts[0][0].astype(np.float64) + parts[1][0].astype(np.float64)
    assert (np.abs(added - ref["A"]) <= BW_TAU * (ref["k"] + BW_C)[:, None] * ref["M"] + BW_ATOL).all()
    assert np.allclose(parts[0][1]["A"] + parts[1][1]["A"], ref["A"], rtol=1e-12, atol=0)


# ---- nothing rendered, an empty band, refusals -------------------------------------------------------------------------------
def test_nothing_rendered_and_an_empty_band_write_zeros():
    import contrib_ref
    scene, cam = contrib_ref.edge_scene()
    off = {k: v.copy() for k, v in scene.items()}
    off["means3D"][:, 0] += 500.0                            # every splat far off the frame: R == 0
    r = _rasterizer(off, cam)
    r.draw(cam)
    assert r.last_num_rendered == 0
    got = _call(r, cam)
    assert (got.view(np.uint32) == 0).all()
    r = _rasterizer(scene, cam)
    r.draw(cam, tile_rows=(1, 1))
    got = _call(r, cam, tile_rows=(1, 1))
    assert (got.view(np.uint32) == 0).all()


def test_every_refusal_again_with_a_device():
    import torch
    import contrib_ref
    from gsrast_amd import _capi
    from test_absgrad_cpu import REFUSALS, refused_untouched
    scene, cam = contrib_ref.edge_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam)
    for case in REFUSALS:                                    # (decided before any HIP call: the addresses are never read)
        refused_untouched(case)
    # through the Python layer: a frame whose sorted lists were skipped; the output stays as it was, the scratch is dropped
    gc = torch.from_numpy(R.pixel_gradients(cam)[0]).to(DEV)
    _call(r, cam)
    assert "absgrad_sums_f64" in r._bw.scratch
    r.draw(cam, plan="blocks", sorted_lists=False)
    assert r.last_plan == "blocks" and not r.last_lists_written
    out = torch.full((r.num_gaussians, 2), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.GsrError) as e:
        r.absgrad(gc, into=out)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG and bool((out == SENTINEL).all())
    assert "absgrad_sums_f64" not in r._bw.scratch
    # ... and the next frame is served again
    _draw_and_check(r, scene, cam, what="after a refusal")


# ---- through autograd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_frame_slot_with_absgrad(profile):
    import torch
    from gsrast_amd.autograd import FrameSlot, render
    from gsrast_amd.densify import DensityStats
    from test_gpu_autograd import BG, DRAW, RAW, _cam, _kw, _params, _rasterizer as _rast, _same_bits, _weights
    wt, wdt, w_np, wd_np = _weights()
    cam = _cam(1)
    grads = {}
    for name, slot in (("abs", FrameSlot(absgrad=True)), ("plain", FrameSlot())):
        params, rast = _params(profile), _rast()
        color, dmap, _ = render(params, rast, cam, radii_slot=slot, depth=True, **_kw(profile), **DRAW)
        ((wt * color).sum() + (wdt * dmap).sum()).backward()
        grads[name] = [getattr(params, k).grad for k in RAW]
        if name == "plain":
            assert slot.abs_dL_dmean2D is None and "absgrad_sums_f64" not in rast._bw.scratch      # nothing launched or allocated
            continue
        n = params.num_gaussians
        got = slot.abs_dL_dmean2D
        assert got.dtype == torch.float32 and tuple(got.shape) == (n, 2) and got.data_ptr() != slot.dL_dmean2D.data_ptr()
        # the same frame by hand, on the rasterizer that still holds it, and both against the joint reference
        hand = rast.absgrad(wt, dL_ddepth=wdt, depth=True, semantics=profile)
        assert hand.data_ptr() != got.data_ptr()
        st = _state(rast)
        d = R.depth_values(rast.means3D.detach().cpu().numpy(), rast._view.detach().cpu().numpy())
        ref = R.frame_absgrad(st, rast.width, rast.height, BG, w_np, wd_np, d, None, R.T_CUTOFF[profile])
        _check(got.cpu().numpy(), ref, f"autograd {profile}, slot")
        _check(hand.cpu().numpy(), ref, f"autograd {profile}, by hand")
        assert bool((got >= 0).all()) and not bool(got[slot.radii <= 0].any())
        # DensityStats.update(absgrad=True) is gsr_densify_accumulate fed that array
        a, b, c = (DensityStats(n, DEV) for _ in range(3))
        a.update(slot, rast.width, rast.height, absgrad=True)
        fed = FrameSlot()
        fed.radii, fed.dL_dmean2D = slot.radii, slot.abs_dL_dmean2D
        b.update(fed, rast.width, rast.height)
        c.update(slot, rast.width, rast.height)
        for k in ("grad_accum", "denom", "max_radii"):
            assert _same_bits(getattr(a, k), getattr(b, k)), k
        assert not _same_bits(a.grad_accum, c.grad_accum) and bool((a.grad_accum >= c.grad_accum * (1 - 1e-5)).all())
    torch.cuda.synchronize()
    for x, y, k in zip(grads["abs"], grads["plain"], RAW):
        assert _same_bits(x, y), k


def test_five_training_steps_with_a_densification_half_way():
    import torch
    from gsrast_amd.autograd import FrameSlot, GaussianParams, render
    from gsrast_amd.densify import DensityStats, densify_and_prune
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer as _rast
    profile = "inria"
    cam, rast = _cam(1), _rast()
    raw = _raw_scene(profile)
    make = lambda: GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major", device=DEV)
    with torch.no_grad():
        target = render(make(), rast, cam, **_kw(profile))[0]
    params = make()
    with torch.no_grad():
        params.xyz.add_(0.02 * torch.randn(params.xyz.shape, generator=torch.Generator().manual_seed(5)).to(DEV))
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": 1e-3} for k in RAW])
    slot, stats = FrameSlot(absgrad=True), DensityStats(params.num_gaussians, DEV)
    losses, counts = [], None
    for step in range(5):
        if step == 2:
            seen = stats.denom > 0
            mean = (stats.grad_accum[seen] / stats.denom[seen]).median()
            _, counts = densify_and_prune(params, opt, stats, max_grad=float(mean), extent=4.0, generator=torch.Generator().manual_seed(3))
        n = params.num_gaussians
        opt.zero_grad(set_to_none=True)
        loss = (render(params, rast, cam, radii_slot=slot, **_kw(profile))[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        loss.backward()
        assert tuple(slot.abs_dL_dmean2D.shape) == (n, 2) and tuple(slot.dL_dmean2D.shape) == (n, 2)
        assert bool(torch.isfinite(slot.abs_dL_dmean2D).all()) and bool((slot.abs_dL_dmean2D >= 0).all())
        opt.step(slot.radii)
        stats.update(slot, rast.width, rast.height, absgrad=True)
    torch.cuda.synchronize()
    kept, clones, splits, total = counts
    print(f"[absgrad training] {len(raw['xyz'])} Gaussians -> {total}: {kept} kept, {clones} clones, {splits} split; losses {losses}")
    assert clones + splits > 0 and params.num_gaussians == total and all(np.isfinite(losses))
    assert all(bool(torch.isfinite(getattr(params, k)).all()) for k in RAW)
