"""GPU: per-Gaussian contribution statistics, gsr_contribution (include/gsrast_amd_contrib.h; gsrast_amd.contrib). The reference is
tests/contrib_ref.py's float32 replay over the forward state read back from the GPU (map_geometry_state / map_image_state /
map_binning_state); every comparison with it is bit for bit on all four arrays. tests/test_contrib_cpu.py establishes what
that rests on: the replay's finalT / nContrib are the oracle's bit for bit on every scene used here, and the scenes hold
the cases (Gaussians with tiles that nothing blends, pixels that stop on the cut-off, pixels that blend nothing)."""
import ctypes as C

import numpy as np
import pytest

import contrib_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_TORCH = {"weight_sum": "int64", "weight_max": "int32", "pixels": "int64", "dominant": "int64"}


def _rasterizer(scene, cam):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, device=DEV)
    r.configure_from_scene(scene)
    return r


def _state(r):
    """The forward state of r's last draw(), as numpy arrays under the oracle's names."""
    g, im = r.map_geometry_state(), r.map_image_state()
    return {"means2D": g["means2D"].cpu().numpy(), "conicOpacity": g["conicOpacity"].cpu().numpy(), "radii": g["radii"].cpu().numpy(),
            "ranges": im["ranges"].cpu().numpy().view(np.uint32), "nContrib": im["nContrib"].cpu().numpy().view(np.uint32),
            "finalT": im["finalT"].cpu().numpy(),
            "values": (r.map_binning_state()["values"].cpu().numpy().view(np.uint32) if r.last_num_rendered else np.zeros(0, np.uint32))}


def _zeros(n, names=R.NAMES, fill=0):
    import torch
    return {k: torch.full((n,), fill, dtype=getattr(torch, _TORCH[k]), device=DEV) for k in names}


def _run(r, arrays, semantics="gscuda", receipt=None, flags=0):
    """One gsr_contribution call for r's last draw() (or `receipt`) into `arrays` {name: tensor}, on the current stream."""
    from gsrast_amd import _capi
    from gsrast_amd.contrib import contribution_args
    a = contribution_args(r, receipt if receipt is not None else r.last_receipt, semantics, {k: t.data_ptr() for k, t in arrays.items()})
    a.flags |= flags
    _capi.call("gsr_contribution", C.byref(a), device=r.device)
    return a


def _host(arrays):
    import torch
    torch.cuda.synchronize()
    return {k: t.cpu().numpy().view(R.DTYPES[k]) for k, t in arrays.items()}


def _assert_equal(got, ref, what, names=R.NAMES):
    for k in names:
        bad = np.nonzero(got[k] != ref[k])[0]
        assert bad.size == 0, (what, k, f"{bad.size} rows differ", bad[:8], got[k][bad[:8]], ref[k][bad[:8]])


def _draw_and_check(r, cam, semantics="gscuda", what="", **draw):
    r.draw(cam, semantics=semantics, sh_degree=0, **draw)
    ref = R.of_state(_state(r), cam, semantics)
    got = _zeros(r.num_gaussians)
    _run(r, got, semantics)
    got = _host(got)
    _assert_equal(got, ref, what)
    return got, ref


# ---- one 16 x 16 tile: the wave's batch of 64 and the round of 256 -----------------------------------------------------------
@pytest.mark.parametrize("opaque", [False, True], ids=["faint", "opaque"])
@pytest.mark.parametrize("length", R.LIST_LENGTHS)
def test_one_tile_lists_of_every_length(length, opaque):
    scene, cam = R.one_tile_scene(length, opaque)
    r = _rasterizer(scene, cam)
    got, ref = _draw_and_check(r, cam, what=f"length {length}")
    st = _state(r)
    assert int(st["ranges"][0, 1]) - int(st["ranges"][0, 0]) == length
    assert int(ref["nContrib"].max()) == length if not opaque else ref["pixels"].sum() > 0
    assert got["pixels"].sum() > 0 and got["weight_max"].max() > 0


# ---- 40 x 24: partial edge tiles in both directions ------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_edge_tiles_both_semantics_and_both_plans(semantics):
    scene, cam = R.edge_scene()
    r = _rasterizer(scene, cam)
    a, ref = _draw_and_check(r, cam, semantics, f"{semantics} sort", plan="sort")
    assert r.last_plan == "sort"
    b, _ = _draw_and_check(r, cam, semantics, f"{semantics} blocks", plan="blocks")
    assert r.last_plan == "blocks" and r.last_lists_written
    _assert_equal(a, b, "sort against blocks")
    vis = _state(r)["radii"] > 0
    assert (vis & (ref["pixels"] == 0)).any() and ref["stopped"].any() and (ref["nContrib"] == 0).any()


# ---- 128 x 128: 64 tiles add into one row; bands -----------------------------------------------------------------------------
def test_screen_filling_gaussian_and_bands_of_tile_rows():
    scene, cam = R.fill_scene()
    r = _rasterizer(scene, cam)
    whole, ref = _draw_and_check(r, cam, what="whole frame")
    assert int(whole["pixels"][0]) > 6400
    full_state = _state(r)
    # a band: rows 1 and 2 alone, against the reference restricted to them
    r.draw(cam, tile_rows=(1, 3))
    band = _zeros(r.num_gaussians)
    _run(r, band)
    band = _host(band)
    ref_band = R.of_state(full_state, cam, tile_rows=(1, 3))
    _assert_equal(band, ref_band, "rows 1-2")
    assert 0 < int(band["pixels"].sum()) < int(whole["pixels"].sum())
    # two bands accumulated into the same arrays: the whole frame
    acc = _zeros(r.num_gaussians)
    for rows in ((0, 3), (3, 8)):
        r.draw(cam, tile_rows=rows)
        _run(r, acc)
    _assert_equal(_host(acc), whole, "two bands against the whole frame")


# ---- accumulation over calls -----------------------------------------------------------------------------------------------
def test_two_cameras_add_into_arrays_that_start_non_zero():
    import torch
    scene, cams = R.two_view_scene()
    r = _rasterizer(scene, cams[0])
    n = r.num_gaussians
    rng = np.random.default_rng(5)
    start = {"weight_sum": rng.integers(0, 1 << 40, n).astype(np.uint64), "weight_max": rng.integers(0, 1 << 31, n).astype(np.uint32),
             "pixels": rng.integers(0, 1000, n).astype(np.uint64), "dominant": rng.integers(0, 1000, n).astype(np.uint64)}
    start["weight_max"][::2] = 0
    acc = {k: torch.from_numpy(v.view(np.dtype(_TORCH[k]))).to(DEV) for k, v in start.items()}
    want = dict(start)
    refs = []
    for cam in cams:
        r.draw(cam)
        refs.append(R.of_state(_state(r), cam))
        want = R.add(want, refs[-1])
        _run(r, acc)
    got = _host(acc)
    _assert_equal(got, want, "two views over a start")
    assert (refs[0]["pixels"] != refs[1]["pixels"]).any()
    kept_max = (got["weight_max"] == start["weight_max"]) & (start["weight_max"] > 0)
    assert kept_max.any() and (got["weight_max"] > start["weight_max"]).any()          # the larger of the two, either way


def test_each_output_alone_sentinels_and_untouched_chunks():
    import torch
    scene, cam = R.edge_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam)
    ref = R.of_state(_state(r), cam)
    n, guard = r.num_gaussians, 8
    torch.cuda.synchronize()
    before = [c.tensor.clone() for c in (r.geom, r.image, r.binning)]
    for k in R.NAMES:
        dtype = getattr(torch, _TORCH[k])
        buf = torch.full((n + 2 * guard,), -3, dtype=dtype, device=DEV)
        buf[guard:guard + n] = 0
        _run(r, {k: buf[guard:guard + n]})
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert (host[:guard] == -3).all() and (host[guard + n:] == -3).all(), k
        _assert_equal({k: host[guard:guard + n].view(R.DTYPES[k])}, ref, f"{k} alone", names=(k,))
    for c, b in zip((r.geom, r.image, r.binning), before):
        assert torch.equal(c.tensor, b)


def test_two_runs_on_two_streams_give_the_same_bits():
    import torch
    scene, cam = R.fill_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam)
    runs = [_zeros(r.num_gaussians), _zeros(r.num_gaussians)]
    torch.cuda.synchronize()
    for arrays in runs:
        with torch.cuda.stream(torch.cuda.Stream(device=DEV)):
            _run(r, arrays)
    a, b = _host(runs[0]), _host(runs[1])
    _assert_equal(a, b, "two streams")
    assert a["dominant"].sum() > 0


def test_profile_flag_times_the_pass():
    from gsrast_amd import _capi
    scene, cam = R.edge_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam)
    assert _run(r, _zeros(r.num_gaussians)).stage_ms == 0.0
    assert _run(r, _zeros(r.num_gaussians), flags=_capi.GSR_FLAG_PROFILE).stage_ms > 0.0


# ---- refusals and the empty frame ------------------------------------------------------------------------------------------------
def test_nothing_rendered_is_ok_and_writes_nothing():
    from helpers import pixel_splats
    cam = R.one_tile_scene(63, False)[1]
    scene = pixel_splats(cam, [-300.0, -250.0], [4.0, 8.0], [0.0, 0.5], [1.0, 1.0], [0.5, 0.9], np.zeros((2, 3)))
    r = _rasterizer(scene, cam)
    r.draw(cam)
    assert r.last_num_rendered == 0 and int(r.last_receipt.num_rendered) == 0
    arrays = _zeros(2, fill=5)
    _run(r, arrays)
    assert all((v == 5).all() for v in _host(arrays).values())


def test_refused_after_a_draw_without_sorted_lists():
    from gsrast_amd import _capi
    from gsrast_amd.contrib import ContributionStats
    scene, cam = R.edge_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam, plan="blocks", sorted_lists=False)
    assert r.last_plan == "blocks" and not r.last_lists_written
    arrays = _zeros(r.num_gaussians, fill=9)
    with pytest.raises(_capi.GsrError) as e:
        _run(r, arrays)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG
    assert all((v == 9).all() for v in _host(arrays).values())
    stats = ContributionStats(r.num_gaussians, DEV)
    with pytest.raises(ValueError, match="sorted"):
        stats.update(r)
    assert stats.frames == 0 and not any(bool(t.any()) for t in stats.raw.values())


# ---- against the forward's own outputs, with no reference ------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
@pytest.mark.parametrize("which", ["edge", "fill"])
def test_identities_with_the_forwards_own_outputs(which, semantics):
    scene, cam = R.edge_scene() if which == "edge" else R.fill_scene()
    r = _rasterizer(scene, cam)
    r.draw(cam, semantics=semantics, sh_degree=0)
    arrays = _zeros(r.num_gaussians)
    _run(r, arrays, semantics)
    got, st = _host(arrays), _state(r)
    assert int(got["dominant"].sum()) == int((st["nContrib"] > 0).sum())
    total = float(got["weight_sum"].astype(np.float64).sum() * 2.0 ** -32)
    opacity = float((1.0 - st["finalT"].astype(np.float64)).sum())
    # each blended record contributes at most about three float32 roundings of magnitude <= 2^-24 T to the pixel's telescoping
    # sum 1 - finalT = sum alpha_k T_k, plus 2^-32 of truncation
    bound = 2.0 ** -21 * (float(got["pixels"].sum()) + cam.width * cam.height)
    print(f"[contrib] {which} {semantics}: |sum weight - sum (1 - finalT)| = {abs(total - opacity):.3e}: {abs(total - opacity) / bound:.3f} of the bound {bound:.3e}")
    assert opacity > 10.0 and abs(total - opacity) <= bound


# ---- gsrast_amd.contrib ------------------------------------------------------------------------------------------------------
def _raw(scene):
    op = np.clip(scene["opacities"].astype(np.float64), 1e-6, 1 - 1e-6)
    return (scene["means3D"][:, :3].copy(), np.log(op / (1 - op)).astype(np.float32), np.log(scene["scales"][:, :3]).astype(np.float32),
            scene["rotations"].copy(), scene["shs"].copy())


def _params(scene):
    from gsrast_amd.autograd import GaussianParams
    return GaussianParams.from_raw(*_raw(scene), device=DEV)


def _blank_rasterizer(cam):
    from gsrast_amd.rasterizer import SplatRasterizer
    return SplatRasterizer(cam.width, cam.height, device=DEV)


def test_stats_update_after_render_and_its_properties():
    import torch
    from gsrast_amd.autograd import render
    from gsrast_amd.contrib import ContributionStats
    scene, cam = R.edge_scene()
    params, r = _params(scene), _blank_rasterizer(cam)
    stats = ContributionStats(params.num_gaussians, DEV)
    with torch.no_grad():
        render(params, r, cam)
        stats.update(r)
        ref = R.of_state(_state(r), cam)
        render(params, r, cam)
        stats.update(r)
    assert stats.frames == 2
    twice = R.add(ref, ref)
    _assert_equal({k: t.cpu().numpy().view(R.DTYPES[k]) for k, t in stats.raw.items()}, twice, "two updates")
    assert stats.weight_sum.dtype == torch.float64 and stats.weight_max.dtype == torch.float32
    assert stats.pixels.dtype == torch.int64 and stats.dominant.dtype == torch.int64
    assert np.array_equal(stats.weight_sum.cpu().numpy(), twice["weight_sum"].astype(np.float64) * 2.0 ** -32)
    assert np.array_equal(stats.weight_max.cpu().numpy(), (twice["weight_max"].astype(np.float64) * 2.0 ** -32).astype(np.float32))
    assert float(stats.weight_max.max()) > 0.5          # (beyond the sign bit of an int32 view: read unsigned)
    assert np.array_equal(stats.pixels.cpu().numpy(), twice["pixels"].astype(np.int64))
    stats.reset()
    assert stats.frames == 0 and stats.num_gaussians == params.num_gaussians and not bool(stats.raw["pixels"].any())
    stats.reset(7)
    assert stats.num_gaussians == 7
    # a subset: the others are neither kept nor computed
    some = ContributionStats(params.num_gaussians, DEV, what=("weight_max",))
    with torch.no_grad():
        render(params, r, cam)
        some.update(r)
    assert set(some.raw) == {"weight_max"} and np.array_equal(some.raw["weight_max"].cpu().numpy().view(np.uint32), ref["weight_max"])
    with pytest.raises(AttributeError):
        some.pixels


def test_stats_update_between_render_and_backward_leaves_the_gradients_alone():
    import torch
    from gsrast_amd.autograd import render
    from gsrast_amd.contrib import ContributionStats
    scene, cam = R.edge_scene()
    weight = torch.from_numpy(np.random.default_rng(3).normal(size=(3, cam.height, cam.width)).astype(np.float32)).to(DEV)
    grads = []
    for with_stats in (False, True):
        params, r = _params(scene), _blank_rasterizer(cam)
        color = render(params, r, cam)[0]
        if with_stats:
            stats = ContributionStats(params.num_gaussians, DEV)
            stats.update(r)
            assert bool(stats.pixels.any())
        (weight * color).sum().backward()
        grads.append([getattr(params, k).grad.clone() for k in ("xyz", "opacity_logit", "log_scale", "rotation", "shs")])
    for i, (a, b) in enumerate(zip(*grads)):
        assert torch.equal(a, b)
        assert i == 3 or bool(a.abs().sum() > 0)          # (round splats: no gradient reaches the rotations)


def test_stats_update_refuses_before_launching():
    import torch
    from gsrast_amd.contrib import ContributionStats
    scene, cam = R.edge_scene()
    r = _rasterizer(scene, cam)
    stats = ContributionStats(r.num_gaussians, DEV)
    with pytest.raises(ValueError, match="no frame"):
        stats.update(r)
    r.draw(cam)
    with pytest.raises(ValueError, match="rows"):
        ContributionStats(r.num_gaussians + 1, DEV).update(r)
    with pytest.raises(ValueError, match="semantics"):
        stats.update(r, semantics="upstream")
    with pytest.raises(ValueError):
        ContributionStats(r.num_gaussians, "cpu").update(r)
    for what in ((), ("weights",), ("pixels", "pixels")):
        with pytest.raises(ValueError):
            ContributionStats(4, DEV, what=what)
    assert stats.frames == 0 and not any(bool(t.any()) for t in stats.raw.values())
    stats.update(r)
    assert stats.frames == 1 and bool(stats.pixels.any())


def _optimiser(kind, params):
    import torch
    from gsrast_amd.optim import GaussianAdam
    groups = [{"params": [getattr(params, k)], "lr": 1e-3 * (i + 1)} for i, k in enumerate(("xyz", "opacity_logit", "log_scale", "rotation", "shs"))]
    return None if kind == "none" else (GaussianAdam(groups) if kind == "gaussian_adam" else torch.optim.Adam(groups))


@pytest.mark.parametrize("kind", ["gaussian_adam", "torch_adam", "none"])
def test_prune_rows_against_numpy_masks_and_a_step_after(kind):
    import torch
    from gsrast_amd.autograd import render
    from gsrast_amd.contrib import prune_rows
    from gsrast_amd.densify import RAW
    scene, cam = R.edge_scene()
    params, r = _params(scene), _blank_rasterizer(cam)
    opt = _optimiser(kind, params)
    weight = torch.from_numpy(np.random.default_rng(4).normal(size=(3, cam.height, cam.width)).astype(np.float32)).to(DEV)

    def step():
        if opt is not None:
            opt.zero_grad(set_to_none=True)
        (weight * render(params, r, cam)[0]).sum().backward()
        if opt is not None:
            opt.step()
    step()
    step()
    n = params.num_gaussians
    keep = np.random.default_rng(6).uniform(size=n) < 0.6
    keep[:3] = (False, True, False)
    before = {k: getattr(params, k).detach().cpu().numpy().copy() for k in RAW}
    moments = {k: {m: opt.state[getattr(params, k)][m].cpu().numpy().copy() for m in ("exp_avg", "exp_avg_sq")} for k in RAW} if opt else {}
    steps = {k: opt.state[getattr(params, k)]["step"] for k in RAW} if opt else {}
    # refusals first: nothing is replaced
    old = [getattr(params, k) for k in RAW]
    for bad in (torch.from_numpy(keep.astype(np.uint8)).to(DEV), torch.from_numpy(keep[:-1]).to(DEV), torch.from_numpy(keep), keep):
        with pytest.raises(ValueError, match="keep"):
            prune_rows(params, opt, bad)
    assert all(getattr(params, k) is p for k, p in zip(RAW, old))
    # all True: nothing launched, nothing replaced
    src = prune_rows(params, opt, torch.ones(n, dtype=torch.bool, device=DEV))
    assert src.cpu().numpy().tolist() == list(range(n)) and all(getattr(params, k) is p for k, p in zip(RAW, old))
    src = prune_rows(params, opt, torch.from_numpy(keep).to(DEV))
    rows = np.nonzero(keep)[0]
    assert src.dtype == torch.int32 and np.array_equal(src.cpu().numpy(), rows)
    assert params.num_gaussians == len(rows) < n
    for k in RAW:
        p = getattr(params, k)
        assert isinstance(p, torch.nn.Parameter) and p.requires_grad and p.grad is None
        assert np.array_equal(p.detach().cpu().numpy(), before[k][rows]), k
        if opt is not None:
            assert any(q is p for g in opt.param_groups for q in g["params"]) and old[RAW.index(k)] not in opt.state
            for m in ("exp_avg", "exp_avg_sq"):
                assert np.array_equal(opt.state[p][m].cpu().numpy(), moments[k][m][rows]), (k, m)
                assert np.abs(moments[k][m]).sum() > 0
            assert opt.state[p]["step"] is steps[k] or opt.state[p]["step"] == steps[k]
    step()                                       # a training step at the new row count
    for k in RAW:
        assert getattr(params, k).shape[0] == len(rows) and bool(torch.isfinite(getattr(params, k)).all())
        assert getattr(params, k).grad.shape[0] == len(rows)


def test_end_to_end_pruning_what_nothing_blended_leaves_both_views_as_they_were():
    import torch
    from gsrast_amd.autograd import render
    from gsrast_amd.contrib import ContributionStats, prune_rows
    scene, cams = R.two_view_scene()
    params = _params(scene)
    rasts = [_blank_rasterizer(cam) for cam in cams]
    stats = ContributionStats(params.num_gaussians, DEV)
    before, had_tiles = [], np.zeros(params.num_gaussians, bool)
    with torch.no_grad():
        for r, cam in zip(rasts, cams):
            color = render(params, r, cam)[0]
            stats.update(r)
            st = _state(r)
            # no pixel of either view stops on the cut-off: what is removed below was no pixel's stopping record either
            assert not R.of_state(st, cam)["stopped"].any()
            had_tiles |= st["radii"] > 0
            before.append((color.clone(), r.map_image_state()["finalT"].clone()))
        assert stats.frames == 2
        keep = stats.pixels > 0
        removed = ~keep.cpu().numpy()
        assert int((removed & had_tiles).sum()) > 0            # Gaussians that had tiles in a view and did nothing to either
        src = prune_rows(params, None, keep)
        assert params.num_gaussians == int(keep.sum()) == len(src) < len(removed)
        for r, cam, (color, final_t) in zip(rasts, cams, before):
            again = render(params, r, cam)[0]
            assert torch.equal(again, color) and torch.equal(r.map_image_state()["finalT"], final_t)
            assert bool((final_t < 1.0).any())
