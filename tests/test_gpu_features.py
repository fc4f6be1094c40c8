"""GPU: N-channel feature maps of a drawn frame (include/gsrast_amd_features.h; SplatRasterizer.render_features,
.features_backward, .backward(features=...), autograd.rasterize / render(features=...)). The references are
tests/features_ref.py's — the float32 replay for the forward, bit for bit, and the float64 walk over the forward state read back
from the GPU for the backward; tests/test_features_cpu.py pins both to the project's oracle.

Acceptance of every gradient, per Gaussian and component, is the render backward's rule of tests/helpers.py, unchanged:
    |got - ref| <= BW_TAU (k + BW_C [+ tiles]) M + BW_ATOL, and a row nothing blended is +0.0 bit for bit.
Worst |err| / ((k + BW_C) M) measured on one MI355X (the bound allows BW_TAU = 1.1e-7; every case prints its own): dL_dfeatures
2.59e-8 (edge, C = 33; one tile 1.4e-9 at length 1 to 1.8e-8 at 255 to 257; 256 channels 1.3e-8; a band 1.4e-8); the geometry
sums through backward(features=...) 2.29e-8 (C = 3, one tile of 257 faint records) and 7.1e-9 with a background across chunks;
colour + depth + opacity + features in one call 6.8e-9, its dL_dcolors / dL_ddepths / dL_dfeatures 1.8e-8 / 1.9e-8 / 1.7e-8; the
same call on the block scene A13 (per-entry float sums and direct atomics) 2.0e-8, 2.1e-8 / 2.0e-8 / 2.1e-8; against
helpers.oracle_gradients at C = 3 worst 2.0e-8 (edge), against 11 oracle runs added at C = 33 worst 2.6e-8 (edge)."""
import functools

import numpy as np
import pytest

import absgrad_ref as A
import features_ref as R
from helpers import BW_C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
ALL_C = sum(R.CHANNELS)


def _rasterizer(scene, cam, bg=R.BACKGROUND):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, device=DEV, background=bg)
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


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def _columns():
    """Where each C of R.CHANNELS lies in the one [N, ALL_C] feature matrix whose replay / walk serves all of them (the channels
    of a pass do not see each other in the forward or in dL_dfeatures)."""
    out, at = {}, 0
    for c in R.CHANNELS:
        out[c] = slice(at, at + c)
        at += c
    return out


@functools.lru_cache(maxsize=None)
def _frame(name, semantics="gscuda"):
    """One rasterizer per scene with its frame drawn, the state read back, and the references over all channel counts at once,
    computed once and left unchanged."""
    scene, cam = SCENES[name]
    r = _rasterizer(scene, cam)
    r.draw(cam, semantics=semantics, sh_degree=0, plan="sort", tile_history=False)
    st = _state(r)
    n = r.num_gaussians
    feat, bg, g = R.features_of(n, ALL_C), R.background_of(ALL_C), R.gradient_of(cam, ALL_C)
    fw = R.forward(st, feat, bg, cam.width, cam.height, R.T_CUTOFF[semantics])
    assert np.array_equal(fw["nContrib"], st["nContrib"]) and np.array_equal(_bits(fw["finalT"]), _bits(st["finalT"])), name
    bw = R.backward(st, feat, bg, g, cam.width, cam.height, R.T_CUTOFF[semantics])
    return dict(r=r, scene=scene, cam=cam, st=st, feat=feat, bg=bg, g=g, fw=fw, bw=bw)


# ---- 1. the frame's own colours and depth come back bit for bit ---------------------------------------------------------------
VARIANTS = {"sort": dict(plan="sort", deep_tiles=False), "blocks": dict(plan="blocks"), "deep": dict(plan="sort", deep_tiles="all")}


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_colours_and_depth_of_the_frame_bit_for_bit(variant, semantics):
    for name, (scene, cam) in SCENES.items():
        r = _rasterizer(scene, cam)
        for mode in (True, "inverse"):
            r.draw(cam, semantics=semantics, sh_degree=0, tile_history=False, depth=mode, **VARIANTS[variant])
            assert r.last_plan == VARIANTS[variant]["plan"] and r.last_lists_written, (name, r.last_plan)
            colours = r.map_geometry_state()["rgb"].clone()
            out = r.render_features(colours, background=r.background)
            assert np.array_equal(_bits(out), _bits(r.out_color)), (name, variant, semantics, "out_color")
            d = _t(A.depth_values(scene["means3D"], cam.view, inverse=mode == "inverse")[:, None])
            out = r.render_features(d)
            assert np.array_equal(_bits(out[0]), _bits(r.out_depth)), (name, variant, semantics, mode, "out_depth")
            assert float(out.abs().max()) > 0


# ---- 2, 3. random features at every C against the replay; sentinels; the forward state untouched ------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_random_features_at_every_channel_count_against_the_replay(name):
    import torch
    f = _frame(name)
    r, cam = f["r"], f["cam"]
    H, W = cam.height, cam.width
    before = _chunks(r)
    for c, cols in _columns().items():
        for bg in (f["bg"][cols], None):
            buf = torch.full((c + 2, H, W), SENTINEL, dtype=torch.float32, device=DEV)
            out = r.render_features(_t(f["feat"][:, cols]), background=bg, into=buf[1:c + 1])
            assert out.data_ptr() == buf[1:].data_ptr()
            host = buf.cpu().numpy()
            assert (host[0] == SENTINEL).all() and (host[c + 1] == SENTINEL).all(), "a write outside the output"
            want = f["fw"]["out" if bg is not None else "acc"][cols]
            assert np.array_equal(_bits(host[1:c + 1]), _bits(want)), (name, c, "background" if bg is not None else "none")
    after = _chunks(r)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "a chunk was written"


def test_256_channels_on_one_tile():
    import torch
    f = _frame("tile-65-opaque")
    r, cam, n = f["r"], f["cam"], f["r"].num_gaussians
    feat, bg, g = R.features_of(n, 256, seed=3), R.background_of(256, seed=3), R.gradient_of(cam, 256, seed=3)
    out = r.render_features(_t(feat), background=bg)
    want = R.forward(f["st"], feat, bg, cam.width, cam.height)
    assert np.array_equal(_bits(out), _bits(want["out"]))
    got = r.features_backward(_t(feat), _t(g)).cpu().numpy()
    ref = R.backward(f["st"], feat, bg, g, cam.width, cam.height)
    _check_features(got, ref, slice(0, 256), "256 channels")
    assert not bool(r._bw.scratch["feature_sums_f64"].view(torch.int64).any())


# ---- 4, 5, 6. bands, two streams, nothing rendered ----------------------------------------------------------------------------
def test_a_band_of_tile_rows_leaves_the_other_rows_alone():
    import torch
    scene, cam = SCENES["fill"]
    r = _rasterizer(scene, cam)
    rows = (1, 3)
    r.draw(cam, tile_rows=rows, plan="sort", tile_history=False)
    st = _state(r)
    n, c = r.num_gaussians, 9
    feat, bg = R.features_of(n, c), R.background_of(c)
    buf = torch.full((c, cam.height, cam.width), float("nan"), dtype=torch.float32, device=DEV)
    pattern = _bits(buf).copy()
    r.render_features(_t(feat), background=bg, tile_rows=rows, into=buf)
    want = R.forward(st, feat, bg, cam.width, cam.height, tile_rows=rows)["out"]
    got = buf.cpu().numpy()
    y0, y1 = 16 * rows[0], 16 * rows[1]
    assert np.array_equal(_bits(got[:, y0:y1]), _bits(want[:, y0:y1]))
    assert np.array_equal(_bits(got[:, :y0]), pattern[:, :y0]) and np.array_equal(_bits(got[:, y1:]), pattern[:, y1:])
    g = R.gradient_of(cam, c)
    ref = R.backward(st, feat, bg, g, cam.width, cam.height, tile_rows=rows)
    _check_features(r.features_backward(_t(feat), _t(g), tile_rows=rows).cpu().numpy(), ref, slice(0, c), "band 1-3")


def test_two_streams():
    import torch
    frames = [_frame("edge"), _frame("clamp")]
    cols = _columns()[17]
    single = [(f["r"].render_features(_t(f["feat"][:, cols]), background=f["bg"][cols]).clone(),
               f["r"].features_backward(_t(f["feat"][:, cols]), _t(f["g"][cols])).clone()) for f in frames]
    streams = [torch.cuda.Stream(device=DEV) for _ in frames]
    inputs = [(_t(f["feat"][:, cols]), _t(f["g"][cols])) for f in frames]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for f, s, (ft, gt) in zip(frames, streams, inputs):
            with torch.cuda.stream(s):
                outs.append((f["r"].render_features(ft, background=f["bg"][cols], sync=False), f["r"].features_backward(ft, gt, sync=False)))
    torch.cuda.synchronize()
    for i, (o, d) in enumerate(outs):
        assert torch.equal(o, single[i % 2][0])
        _check_features(d.cpu().numpy(), frames[i % 2]["bw"], cols, f"stream {i % 2}")


def test_nothing_rendered_and_an_empty_band_write_the_background_or_zeros():
    import torch
    scene, cam = SCENES["edge"]
    off = {k: v.copy() for k, v in scene.items()}
    off["means3D"][:, 0] += 500.0                            # every splat far off the frame: R == 0
    r = _rasterizer(off, cam)
    r.draw(cam)
    assert r.last_num_rendered == 0
    n, c = r.num_gaussians, 9
    feat, bg, g = _t(R.features_of(n, c)), R.background_of(c), _t(R.gradient_of(cam, c))
    out = r.render_features(feat, background=bg).cpu().numpy()
    assert np.array_equal(_bits(out), _bits(np.broadcast_to(bg[:, None, None], out.shape).copy()))
    assert (_bits(r.render_features(feat)) == 0).all()
    assert (_bits(r.features_backward(feat, g)) == 0).all()
    res = r.backward(torch.zeros((3, cam.height, cam.width), device=DEV), features=(feat, g))
    assert (_bits(res["dL_dfeatures"]) == 0).all() and (_bits(res["dL_dmean2D"]) == 0).all()
    r = _rasterizer(scene, cam)
    r.draw(cam, tile_rows=(1, 1))
    buf = torch.full((c, cam.height, cam.width), SENTINEL, dtype=torch.float32, device=DEV)
    r.render_features(feat, background=bg, tile_rows=(1, 1), into=buf)
    assert bool((buf == SENTINEL).all())
    assert (_bits(r.features_backward(feat, g, tile_rows=(1, 1))) == 0).all()
    # without tile_rows the calls take the receipt's own band, and a new tensor is zeros wherever the band does not reach
    assert (_bits(r.render_features(feat, background=bg)) == 0).all() and (_bits(r.features_backward(feat, g)) == 0).all()
    r.draw(cam, tile_rows=(0, 1))
    out = r.render_features(feat, background=bg).cpu().numpy()
    assert (_bits(out[:, 16:]) == 0).all() and np.array_equal(_bits(out[:, :16]), _bits(r.render_features(feat, background=bg, tile_rows=(0, 1)).cpu().numpy()[:, :16]))
    assert float(np.abs(out[:, :16]).max()) > 0


# ---- 7. dL_dfeatures ----------------------------------------------------------------------------------------------------------
def _check_features(got, ref, cols, what, float_tile_sums=False):
    """Per-channel sums (dL_dfeatures, or dL_dcolors / dL_ddepths of a joint reference) under the bound; float_tile_sums: bool[N],
    the Gaussians whose sums passed through the block feed's per-entry floats (gsr_backward's own colour and depth sums may)."""
    assert got.dtype == np.float32 and np.isfinite(got).all(), what
    none = ref["pixels"] == 0
    assert (_bits(got[none]) == 0).all(), (what, "a row nothing blended must be +0.0 bit for bit")
    part = {"d_chan": ref["d_chan"][:, cols], "M_d_chan": ref["M_d_chan"][:, cols], "k": ref["k"]}
    worst = R.worst_ratio(got, part, "d_chan")
    print(f"[features] {what}: dL_dfeatures, {int((~none).sum())} blended, worst |err| / ((k + {BW_C:g}) M) = {worst:.3e}")
    over = np.abs(got.astype(np.float64) - part["d_chan"]) > R.bound(dict(part, tiles=ref.get("tiles", 0 * ref["k"])), "d_chan", float_tile_sums)
    assert not over.any(), (what, f"{int(over.any(1).sum())} Gaussians over the bound; worst ratio {worst:.3e}")
    return worst


@pytest.mark.parametrize("name", list(SCENES))
def test_feature_gradients_at_every_channel_count(name):
    import torch
    f = _frame(name)
    r = f["r"]
    for c, cols in _columns().items():
        n = r.num_gaussians
        buf = torch.full((n + 2, c), SENTINEL, dtype=torch.float32, device=DEV)
        got = r.features_backward(_t(f["feat"][:, cols]), _t(f["g"][cols]), background=f["bg"][cols], into=buf[1:n + 1])
        host = buf.cpu().numpy()
        assert (host[0] == SENTINEL).all() and (host[n + 1] == SENTINEL).all(), "a write outside the output"
        assert not bool(r._bw.scratch["feature_sums_f64"].view(torch.int64).any()), "the scratch is not left zero"
        assert "sums_f64" not in r._bw.scratch, "features_backward touched backward()'s scratch"
        _check_features(host[1:n + 1], f["bw"], cols, f"{name} C={c}")


# ---- 8, 9, 10. geometry: through backward(features=...) -----------------------------------------------------------------------
GEO = (("dL_dmean2D", "d_mean", slice(0, 2)), ("dL_dconic_opacity", "d_conic", slice(0, 3)), ("dL_dconic_opacity", "d_op", slice(3, 4)),
       ("dL_dcov2D", "d_cov", slice(0, 3)))


def _check_geometry(res, ref, what, float_tile_sums=False, factor=1.0, extra=None):
    """Every per-Gaussian sum of a backward() result against a features_ref.backward reference (factor / extra: the bound
    scaled, or another bound added, where two float evaluations are compared)."""
    none = ref["pixels"] == 0
    worst = 0.0
    for out, key, part in GEO:
        got = res[out].cpu().numpy()[:, part].astype(np.float64)
        assert np.isfinite(got).all() and (got[none] == 0.0).all(), (what, key)
        b = factor * R.bound(ref, key, float_tile_sums) + (extra[key] if extra is not None else 0.0)
        over = np.abs(got - ref[key]) > b
        worst = max(worst, R.worst_ratio(got, ref, key))
        assert not over.any(), (what, key, f"{int(over.any(1).sum())} Gaussians over the bound; worst ratio {R.worst_ratio(got, ref, key):.3e}")
    print(f"[features] {what}: geometry sums, worst |err| / ((k + {BW_C:g}) M) = {worst:.3e}")
    return worst


def _oracle(r, cam, F, G, bg):
    """helpers.oracle_gradients (oracle/backward_np.blend_tile_backward over the GPU's forward state, float32 decisions, float64
    sums, condition scales) of every Gaussian with colours F [N,3], pixel gradient G [3,H,W] and background bg."""
    from helpers import oracle_gradients
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    tiles = [(tx, ty) for ty in range(gy) for tx in range(gx)]
    return oracle_gradients(r, G, bg, tiles, np.arange(r.num_gaussians), 4096, f32_forward=True, magnitudes=True, full_lists=True,
                            colors=np.asarray(F, np.float32), background=tuple(float(v) for v in bg))


def _oracle_superposition(r, cam, F, G, bg):
    """ceil(C / 3) oracle runs over the same lists, added as helpers.depth_superposition adds the depth pass: the blend is linear
    in the (channel, gradient) pairs and so is every condition scale; dL_dcolors becomes the runs' side by side, [N,C]."""
    c = F.shape[1]
    pad = (-c) % 3
    Fp, Gp, bp = np.pad(F, ((0, 0), (0, pad))), np.pad(G, ((0, pad), (0, 0), (0, 0))), np.pad(bg, (0, pad))
    runs = [_oracle(r, cam, Fp[:, j:j + 3], Gp[j:j + 3], bp[j:j + 3]) for j in range(0, c + pad, 3)]
    out = dict(runs[0])
    for key in ("exp", "M"):
        out[key] = {k: sum(run[key][k] for run in runs) for k in runs[0][key] if k != "dL_dcolors"}
        out[key]["dL_dcolors"] = np.concatenate([run[key]["dL_dcolors"] for run in runs], 1)[:, :c]
    assert all(np.array_equal(run["k"], runs[0]["k"]) and np.array_equal(run["pixels"], runs[0]["pixels"]) for run in runs)
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_geometry_of_three_channels_against_the_oracle_and_against_colours(name):
    import torch
    from helpers import assert_backward_per_gaussian, check_backward_chain, gradients_of
    f = _frame(name)
    r, cam, st, scene = f["r"], f["cam"], f["st"], f["scene"]
    n, (H, W) = r.num_gaussians, (cam.height, cam.width)
    cols = _columns()[3]
    F, G = f["feat"][:, cols], f["g"][cols]
    zeros = torch.zeros((3, H, W), device=DEV)
    res = r.backward(zeros, features=(_t(F), _t(G)))
    ref = R.backward(st, F, None, G, W, H)
    _check_geometry(res, ref, f"{name} C=3")
    _check_features(res["dL_dfeatures"].cpu().numpy(), ref, slice(0, 3), f"{name} C=3 via backward()")
    assert (_bits(res["dL_dcolors"]) == 0).all(), "the colour slots are not the feature pass's"
    # the project's float64 oracle itself: colours F, gradient G, zero background
    got = gradients_of(dict(res, dL_dcolors=res["dL_dfeatures"]), np.arange(n))
    assert_backward_per_gaussian(got, _oracle(r, cam, F, G, (0.0, 0.0, 0.0)), what=f"{name} C=3, oracle")
    assert not bool(r._bw.scratch["sums_f64"].view(torch.int64).any()) and not bool(r._bw.scratch["feature_sums_f64"].view(torch.int64).any())
    # the chain below the sums, fed with the GPU's own sums
    host = {k: v.cpu().numpy() for k, v in res.items()}
    geo = {"cov3D": r.map_geometry_state()["cov3D"].cpu().numpy()}
    ids = np.nonzero(ref["free_pixels"] > 0)[0][:40]
    check_backward_chain(host, geo, scene, cam, W, H, ids)
    # the same loss as a colour loss: the scene drawn with colors_precomp = F over a zero background (two float evaluations)
    r2 = _rasterizer(scene, cam, bg=(0.0, 0.0, 0.0))
    r2.draw(cam, colors_precomp=_t(F), plan="sort", tile_history=False)
    res2 = r2.backward(_t(G))
    extra = {key: R.bound(ref, key) for _, key, _ in GEO}
    _check_geometry({k: res2[k] for k in ("dL_dmean2D", "dL_dconic_opacity", "dL_dcov2D")}, ref, f"{name} colours", extra=None)
    for out, key, part in GEO:
        a, b = res[out].cpu().numpy()[:, part].astype(np.float64), res2[out].cpu().numpy()[:, part].astype(np.float64)
        assert (np.abs(a - b) <= 2.0 * extra[key]).all(), (name, key, "against backward(G) of the frame with colors_precomp = F")
    assert (np.abs(res["dL_dfeatures"].cpu().numpy().astype(np.float64) - res2["dL_dcolors"].cpu().numpy())
            <= 2.0 * R.bound(dict(ref, tiles=0 * ref["k"]), "d_chan")).all()


@pytest.mark.parametrize("name", ["tile-257-opaque", "edge", "fill", "clamp"])
def test_geometry_across_chunks_and_with_a_background(name):
    import torch
    from helpers import assert_backward_per_gaussian, gradients_of
    f = _frame(name)
    r, cam, st = f["r"], f["cam"], f["st"]
    zeros = torch.zeros((3, cam.height, cam.width), device=DEV)
    for c in (R.CHUNK + 1, 2 * R.CHUNK + 1):
        cols = _columns()[c]
        F, G, bg = f["feat"][:, cols], f["g"][cols], f["bg"][cols]
        ref = R.backward(st, F, bg, G, cam.width, cam.height)
        res = r.backward(zeros, features=(_t(F), _t(G), bg))
        _check_geometry(res, ref, f"{name} C={c} with a background")
        _check_features(res["dL_dfeatures"].cpu().numpy(), ref, slice(0, c), f"{name} C={c} via backward()")
        if c == 2 * R.CHUNK + 1:         # ... and against the superposition of ceil(C / 3) runs of the project's oracle
            got = gradients_of(dict(res, dL_dcolors=res["dL_dfeatures"]), np.arange(r.num_gaussians))
            assert_backward_per_gaussian(got, _oracle_superposition(r, cam, F, G, bg), what=f"{name} C={c}, oracle runs added")


def _joint_case(r, st, scene, cam, F, G, seed=5):
    gc, gd, ga = A.pixel_gradients(cam, seed)
    d = A.depth_values(scene["means3D"], cam.view)
    chan, bg, g = R.joint_channels(st["rgb"], r.background.cpu().numpy(), gc, F, G, d, gd, ga)
    return (gc, gd, ga), (chan, bg, g)


def test_colour_depth_opacity_and_features_in_one_call():
    import torch
    f = _frame("edge")
    r, cam, st, scene = f["r"], f["cam"], f["st"], f["scene"]
    cols = _columns()[9]
    F, G = f["feat"][:, cols], f["g"][cols]
    (gc, gd, ga), (chan, bg, g) = _joint_case(r, st, scene, cam, F, G)
    ref = R.backward(st, chan, bg, g, cam.width, cam.height)
    kw = dict(dL_ddepth=_t(gd), depth=True, dL_dalpha=_t(ga))
    plain = {k: v.clone() for k, v in r.backward(_t(gc), **kw).items()}
    res = r.backward(_t(gc), features=(_t(F), _t(G)), camera=True, **kw)
    _check_geometry(res, ref, "edge, joint")
    for out, part, what in (("dL_dcolors", slice(0, 3), "colour"), ("dL_ddepths", slice(3, 4), "depth"), ("dL_dfeatures", slice(5, 14), "features")):
        _check_features(res[out].cpu().numpy().reshape(r.num_gaussians, -1), ref, part, f"edge, joint: {what}")
    for k in ("sums_f64", "depth_sums_f64", "feature_sums_f64"):
        assert not bool(r._bw.scratch[k].view(torch.int64).any()), k
    # 10. gsr_backward without features: the same bits before and after feature calls on the same frame
    r.features_backward(_t(F), _t(G))
    again = r.backward(_t(gc), **kw)
    assert all(np.array_equal(_bits(plain[k]), _bits(again[k])) for k in plain)
    # the camera gradients hold the feature term: against a frame whose colours carry it (C = 3: colours F, zero background)
    cols3 = _columns()[3]
    F3, G3 = f["feat"][:, cols3], f["g"][cols3]
    zeros = torch.zeros((3, cam.height, cam.width), device=DEV)
    cam_f = {k: v.clone() for k, v in r.backward(zeros, features=(_t(F3), _t(G3)), camera=True).items() if k in ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")}
    r2 = _rasterizer(scene, cam, bg=(0.0, 0.0, 0.0))
    r2.draw(cam, colors_precomp=_t(F3), plan="sort", tile_history=False)
    cam_c = r2.backward(_t(G3), camera=True)
    for k, v in cam_f.items():
        a, b = v.cpu().numpy().astype(np.float64), cam_c[k].cpu().numpy().astype(np.float64)
        # (two float evaluations of sums over all Gaussians; the gscuda colour does not depend on cam_pos: zeros on both sides)
        assert (np.abs(b).max() > 0 or k == "dL_dcam_pos") and (np.abs(a - b) <= 1e-4 * np.abs(b).max()).all(), (k, a, b)


def test_joint_call_on_a_frame_of_several_blocks():
    """Colour + depth + opacity + features in one call on helpers.block_scene_a (A13: thirteen per-entry floats fit), fed from
    the block lists with the sorted lists beside: blocks whose thirteen sums pass through the per-entry floats
    (flush_block_acc_kernel<DEPTH>) and a block on the direct double atomics in one launch of
    render_backward_kernel<DEPTH, ALPHA> (asserted from the forward state), the feature pass's seeded double sums under both."""
    import torch
    import helpers as Hh
    scene, cam = Hh.block_scene_a(Hh.BLOCK_SCENE_A_FILL["A13"])
    r = _rasterizer(scene, cam, bg=(0.3, 0.1, 0.6))
    r.draw(cam, plan="sort", tile_history=False)
    facts = Hh.block_feed_facts(Hh.host_snapshot(r), depth=True)
    assert facts["k_acc"] == 13
    Hh.assert_block_ways(facts, {(0, 0): "direct", (1, 0): "per_entry", (2, 0): "per_entry", (0, 1): "per_entry", (1, 1): "per_entry",
                                 (2, 1): "per_entry"}, "A13 with the depth channel")
    r.draw(cam, plan="blocks", overlap_emit=True, tile_history=False)
    assert r.last_plan == "blocks" and r.last_lists_written and not r.last_blend_from_lists
    st = _state(r)
    n = r.num_gaussians
    F, G = R.features_of(n, 3), R.gradient_of(cam, 3)
    gc, gd = Hh.block_scene_gradient(cam.width, cam.height)
    ga = np.random.default_rng(23).normal(size=(cam.height, cam.width)).astype(np.float32)
    d = A.depth_values(scene["means3D"], cam.view)
    chan, bg, g = R.joint_channels(st["rgb"], r.background.cpu().numpy(), gc, F, G, d, gd, ga)
    ref = R.backward(st, chan, bg, g, cam.width, cam.height, prefix=True)
    on = ref["n_contrib"] >= 0
    assert np.array_equal(ref["n_contrib"][on], st["nContrib"].astype(np.int64)[on])
    res = r.backward(_t(gc), dL_ddepth=_t(gd), depth=True, dL_dalpha=_t(ga), features=(_t(F), _t(G)))
    floats = Hh.float_sum_gaussians(facts, np.arange(n))
    assert floats.any() and not floats.all()
    _check_geometry(res, ref, "block scene A13, joint", float_tile_sums=floats)
    _check_features(res["dL_dcolors"].cpu().numpy(), ref, slice(0, 3), "block scene A13: colour", float_tile_sums=floats)
    _check_features(res["dL_ddepths"].cpu().numpy().reshape(n, 1), ref, slice(3, 4), "block scene A13: depth", float_tile_sums=floats)
    _check_features(res["dL_dfeatures"].cpu().numpy(), ref, slice(5, 8), "block scene A13: features")
    for k in ("sums_f64", "depth_sums_f64", "feature_sums_f64"):
        assert not bool(r._bw.scratch[k].view(torch.int64).any()), k


# ---- 11. autograd -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_autograd_feature_map(profile):
    import torch
    from gsrast_amd.autograd import FrameSlot, render
    from test_gpu_autograd import DRAW, RAW, _cam, _kw, _params, _rasterizer as _rast, _same_bits, _weights
    wt, wdt, _, _ = _weights()
    cam = _cam(1)
    c = 9
    n = _params(profile).num_gaussians
    F0 = _t(R.features_of(n, c))
    Gw = _t(R.gradient_of(cam, c))
    # a colour-only loss: the same bits with and without features=
    runs = {}
    for with_f in (False, True):
        params, rast = _params(profile), _rast()
        F = F0.clone().requires_grad_(True)
        out = render(params, rast, cam, **_kw(profile), **DRAW, **({"features": F} if with_f else {}))
        assert len(out) == (4 if with_f else 3)
        (wt * out[0]).sum().backward()
        runs[with_f] = (out[0].detach().clone(), [getattr(params, k).grad.clone() for k in RAW])
        if with_f:
            assert tuple(out[3].shape) == (c, rast.height, rast.width) and F.grad is None
            assert np.array_equal(_bits(out[3]), _bits(rast.render_features(F0)))
    assert _same_bits(runs[False][0], runs[True][0]) and all(_same_bits(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    # a loss on the feature map alone, with antialiasing, a FrameSlot and the depth term beside it: against the hand-run path
    for aa in (False, True):
        params, rast, slot = _params(profile), _rast(), FrameSlot()
        F = F0.clone().requires_grad_(True)
        color, dmap, omap, fmap = render(params, rast, cam, depth=True, radii_slot=slot, antialiased=aa, features=F, **_kw(profile), **DRAW)
        ((Gw * fmap).sum() + (wdt * dmap).sum()).backward()
        zeros = torch.zeros_like(color)
        hand = rast.backward(zeros, semantics=profile, dL_ddepth=wdt, depth=True, features=(F0, Gw),
                             outputs=("dL_dmean2D", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dconic_opacity"))
        assert _same_bits(F.grad, hand["dL_dfeatures"]) and _same_bits(slot.dL_dmean2D, hand["dL_dmean2D"])
        only_depth = rast.backward(zeros, semantics=profile, dL_ddepth=wdt, depth=True, outputs=("dL_dmean2D",))
        assert not _same_bits(only_depth["dL_dmean2D"], slot.dL_dmean2D)          # FrameSlot.dL_dmean2D holds the feature term
        assert all(getattr(params, k).grad is not None and bool(torch.isfinite(getattr(params, k).grad).all()) for k in RAW[:4])
        assert bool((params.xyz.grad[slot.radii > 0] != 0).any())
    # nothing but F requires a gradient: the frozen-geometry pass
    params, rast = _params(profile, requires=()), _rast()
    F = F0.clone().requires_grad_(True)
    fmap = render(params, rast, cam, features=F, **_kw(profile), **DRAW)[3]
    (Gw * fmap).sum().backward()
    assert _same_bits(F.grad, rast.features_backward(F0, Gw)) and "sums_f64" not in rast._bw.scratch
    # a stale graph is refused
    params, rast = _params(profile), _rast()
    F = F0.clone().requires_grad_(True)
    fmap = render(params, rast, cam, features=F, **_kw(profile), **DRAW)[3]
    render(params, rast, _cam(2), **_kw(profile), **DRAW)
    with pytest.raises(RuntimeError, match="has drawn another frame"):
        (Gw * fmap).sum().backward()


def test_autograd_with_the_3d_filter_and_five_training_steps():
    import torch
    from gsrast_amd.autograd import FrameSlot, GaussianParams, render
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer as _rast
    profile, c = "inria", 5
    cam, rast = _cam(1), _rast()
    raw = _raw_scene(profile)
    make = lambda: GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major", device=DEV)
    n = len(raw["xyz"])
    filt = torch.full((n,), 0.01, dtype=torch.float32, device=DEV)
    F_true = _t(R.features_of(n, c))
    with torch.no_grad():
        target = render(make(), rast, cam, features=F_true, filter_3d=filt, **_kw(profile))[3]
    params = make()
    with torch.no_grad():
        params.xyz.add_(0.02 * torch.randn(params.xyz.shape, generator=torch.Generator().manual_seed(5)).to(DEV))
    F = torch.nn.Parameter(F_true + 0.3 * _t(R.features_of(n, c, seed=99)))
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": 1e-3} for k in RAW])
    opt_f = torch.optim.Adam([F], lr=2e-2)
    slot, losses = FrameSlot(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        opt_f.zero_grad(set_to_none=True)
        fmap = render(params, rast, cam, radii_slot=slot, features=F, filter_3d=filt, **_kw(profile))[3]
        loss = ((fmap - target) ** 2).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        assert bool(torch.isfinite(F.grad).all()) and bool((F.grad != 0).any()) and params.log_scale.grad is not None
        opt.step(slot.radii)
        opt_f.step()
    torch.cuda.synchronize()
    print(f"[features training] losses {losses}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]


# ---- 12. refusals, with a device ----------------------------------------------------------------------------------------------
def test_every_refusal_again_with_a_device():
    import torch
    from gsrast_amd import _capi
    from test_features_cpu import REFUSALS, refused_untouched
    scene, cam = SCENES["edge"]
    r = _rasterizer(scene, cam)
    r.draw(cam)
    for case in REFUSALS:                                    # (decided before any HIP call: the addresses are never read)
        refused_untouched(case)
    n = r.num_gaussians
    H, W = cam.height, cam.width
    zeros = torch.zeros((3, H, W), device=DEV)
    F, G = _t(R.features_of(n, 3)), _t(R.gradient_of(cam, 3))
    for c in (0, 257):                                       # through the Python layer
        with pytest.raises(_capi.GsrError) as e:
            r.render_features(torch.zeros((n, c), device=DEV))
        assert e.value.code == _capi.GSR_ERR_INVALID_ARG
    with pytest.raises(AssertionError, match="wide_sums"):
        r.backward(zeros, features=(F, G), wide_sums=False)
    r.features_backward(F, G)
    r.backward(zeros, features=(F, G))
    assert "feature_sums_f64" in r._bw.scratch and "sums_f64" in r._bw.scratch
    # a receipt of another size
    other = _rasterizer(*SCENES["fill"])
    other.draw(SCENES["fill"][1])
    with pytest.raises(_capi.GsrError) as e:
        r.render_features(F, receipt=other.last_receipt)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG
    r.features_backward(F, G)                                # (the scratch a refused forward call never touched is still there)
    # a frame whose sorted lists were skipped: refused, the outputs untouched, both scratches dropped
    r.draw(cam, plan="blocks", sorted_lists=False)
    assert r.last_plan == "blocks" and not r.last_lists_written
    out = torch.full((3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.GsrError) as e:
        r.render_features(F, into=out)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG and bool((out == SENTINEL).all())
    with pytest.raises(_capi.GsrError):
        r.backward(zeros, features=(F, G))
    assert "feature_sums_f64" not in r._bw.scratch and "sums_f64" not in r._bw.scratch
    # ... and the next frame is served again
    r.draw(cam)
    assert np.array_equal(_bits(r.render_features(r.map_geometry_state()["rgb"].clone(), background=r.background)), _bits(r.out_color))
