"""GPU: the depth distortion map of a drawn frame (include/gsrast_amd_distortion.h; SplatRasterizer.render_distortion,
.distortion_backward, .backward(distortion=...), autograd.rasterize / render(distortion=...)). The references are
tests/distortion_ref.py's: the float32 restatement of the header for the forward — `out` and the three moment planes bit for bit —
and the float64 walk over the forward state read back from the GPU, handed the GPU's own moments, for the backward;
tests/test_distortion_cpu.py pins both to the brute-force double sum and to finite differences.

Acceptance of every gradient, per Gaussian and component, is the render backward's rule of tests/helpers.py with its constants
unchanged and n — the largest number of records blended into any pixel the Gaussian touches — in place of k:
    |got - ref| <= BW_TAU (n + BW_C) M + BW_ATOL, and a row nothing blended is +0.0 bit for bit.
Every case prints its worst |err| / ((n + BW_C) M); the bound allows BW_TAU = 1.1e-7. Measured on one MI355X, the worst over both
powers and both sets of values, dL_dvalues / the geometry sums: one tile of 1 record 5.4e-10 / 0, of 63 4.0e-9 / 3.7e-9, of 64
9.1e-9 / 3.2e-9, of 65 1.0e-8 / 5.8e-9, of 255 5.7e-9 / 4.3e-9, of 256 5.1e-9 / 4.0e-9, of 257 8.6e-9 / 4.7e-9; edge 6.2e-9 /
6.3e-9; fill 3.6e-9 / 4.5e-9; clamp 6.6e-9 / 4.0e-9; a band of tile rows 3.4e-9 (dL_dvalues); every term in one backward()
0.033 of the sum of the two references' bounds."""
import functools

import numpy as np
import pytest

import absgrad_ref as A
import distortion_ref as R
import features_ref as FR
from helpers import BW_C

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
KINDS = ("depth", "random")
GEO = (("dL_dmean2D", "d_mean", slice(0, 2)), ("dL_dconic_opacity", "d_conic", slice(0, 3)), ("dL_dconic_opacity", "d_op", slice(3, 4)),
       ("dL_dcov2D", "d_cov", slice(0, 3)))
OUTPUTS = ("dL_dmean2D", "dL_dconic_opacity", "dL_dcov2D", "dL_dcolors")


def _rasterizer(scene, cam, bg=A.BACKGROUND):
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


def _values(scene, cam, kind):
    return R.depth_values(scene, cam) if kind == "depth" else R.random_values(scene["means3D"].shape[0])


@functools.lru_cache(maxsize=None)
def _frame(name):
    """One rasterizer per scene with its frame drawn and the state read back, computed once and left unchanged."""
    scene, cam = SCENES[name]
    r = _rasterizer(scene, cam)
    r.draw(cam, semantics="gscuda", sh_degree=0, plan="sort", tile_history=False)
    return dict(r=r, scene=scene, cam=cam, st=_state(r), g=R.gradient_of(cam))


@functools.lru_cache(maxsize=None)
def _forward(name, kind, power):
    f = _frame(name)
    fw = R.forward32(f["st"], _values(f["scene"], f["cam"], kind), power, f["cam"].width, f["cam"].height)
    assert np.array_equal(fw["nContrib"], f["st"]["nContrib"]) and np.array_equal(_bits(fw["finalT"]), _bits(f["st"]["finalT"])), name
    return fw


@functools.lru_cache(maxsize=None)
def _walk(name, kind, power):
    """The float64 walk handed the float32 moments — the restatement's, which the GPU's are bit for bit (asserted by the callers)."""
    f = _frame(name)
    return R.frame_walk(f["st"], _values(f["scene"], f["cam"], kind), power, f["g"], f["cam"].width, f["cam"].height,
                        moments=_forward(name, kind, power)["moments"])


def _check(got, ref, key, what):
    got = np.asarray(got, np.float64).reshape(ref[key].shape)
    none = ref["pixels"] == 0
    assert np.isfinite(got).all() and (got[none] == 0.0).all(), (what, key)
    worst = R.worst_ratio(got, ref, key)
    over = np.abs(got - ref[key]) > R.bound(ref, key)
    assert not over.any(), (what, key, f"{int(over.any(1).sum())} Gaussians over the bound; worst ratio {worst:.3e}")
    return worst


def _check_all(res, ref, what):
    worst = {key: _check(res[out].cpu().numpy()[:, part], ref, key, what) for out, key, part in GEO}
    worst["d_val"] = _check(res["dL_dvalues"].cpu().numpy(), ref, "d_val", what)
    assert (_bits(res["dL_dvalues"].cpu().numpy()[ref["pixels"] == 0]) == 0).all(), (what, "a row nothing blended must be +0.0")
    print(f"[distortion] {what}: worst |err| / ((n + {BW_C:g}) M): dL_dvalues {worst['d_val']:.3e}, geometry "
          f"{max(v for k, v in worst.items() if k != 'd_val'):.3e}")


# ---- 1. out and the moments, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_out_and_moments_bit_for_bit_against_the_restatement(name):
    import torch
    f = _frame(name)
    r, cam = f["r"], f["cam"]
    H, W = cam.height, cam.width
    before = _chunks(r)
    for kind in KINDS:
        vals = _t(_values(f["scene"], cam, kind))
        for power in R.POWERS:
            fw = _forward(name, kind, power)
            buf = torch.full((3, H, W), SENTINEL, dtype=torch.float32, device=DEV)
            out = r.render_distortion(vals, power=power, into=buf[1])
            assert out.data_ptr() == buf[1].data_ptr()
            host = buf.cpu().numpy()
            assert (host[0] == SENTINEL).all() and (host[2] == SENTINEL).all(), "a write outside the output"
            assert np.array_equal(_bits(host[1]), _bits(fw["out"])), (name, kind, power, "out")
            serial, kept_power, mom = r._distortion_moments
            assert serial == int(r.last_receipt.serial) and kept_power == power
            assert np.array_equal(_bits(mom), _bits(fw["moments"])), (name, kind, power, "moments")
            if power == 1:
                assert (_bits(mom[2]) == 0).all()
            assert np.array_equal(_bits(r.render_distortion(vals, power=power)), _bits(fw["out"]))
    after = _chunks(r)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "a chunk was written"


VARIANTS = {"sort": dict(plan="sort", deep_tiles=False), "blocks": dict(plan="blocks")}


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_both_plans_and_both_semantics_bit_for_bit(variant, semantics):
    for name in ("tile-257-opaque", "edge", "clamp"):
        scene, cam = SCENES[name]
        r = _rasterizer(scene, cam)
        r.draw(cam, semantics=semantics, sh_degree=0, tile_history=False, **VARIANTS[variant])
        assert r.last_plan == VARIANTS[variant]["plan"] and r.last_lists_written, (name, r.last_plan)
        st = _state(r)
        vals = _values(scene, cam, "depth")
        for power in R.POWERS:
            fw = R.forward32(st, vals, power, cam.width, cam.height, R.T_CUTOFF[semantics])
            assert np.array_equal(fw["nContrib"], st["nContrib"]), (name, variant, semantics)
            out = r.render_distortion(_t(vals), power=power)
            assert np.array_equal(_bits(out), _bits(fw["out"])), (name, variant, semantics, power)
            assert np.array_equal(_bits(r._distortion_moments[2]), _bits(fw["moments"])), (name, variant, semantics, power)
            assert float(out.abs().max()) > 0


def test_a_band_of_tile_rows_leaves_the_other_rows_alone():
    import torch
    scene, cam = SCENES["fill"]
    r = _rasterizer(scene, cam)
    rows = (1, 3)
    r.draw(cam, tile_rows=rows, plan="sort", tile_history=False)
    st = _state(r)
    vals, g = R.random_values(r.num_gaussians), R.gradient_of(cam)
    y0, y1 = 16 * rows[0], 16 * rows[1]
    for power in R.POWERS:
        buf = torch.full((cam.height, cam.width), float("nan"), dtype=torch.float32, device=DEV)
        pattern = _bits(buf).copy()
        r.render_distortion(_t(vals), power=power, tile_rows=rows, into=buf)
        fw = R.forward32(st, vals, power, cam.width, cam.height, tile_rows=rows)
        got = buf.cpu().numpy()
        assert np.array_equal(_bits(got[y0:y1]), _bits(fw["out"][y0:y1]))
        assert np.array_equal(_bits(got[:y0]), pattern[:y0]) and np.array_equal(_bits(got[y1:]), pattern[y1:])
        mom = r._distortion_moments[2].cpu().numpy()
        assert np.array_equal(_bits(mom[:, y0:y1]), _bits(fw["moments"][:, y0:y1])) and (_bits(mom[:, :y0]) == 0).all() and (_bits(mom[:, y1:]) == 0).all()
        ref = R.frame_walk(st, vals, power, g, cam.width, cam.height, moments=np.nan_to_num(fw["moments"]), tile_rows=rows)
        got = r.distortion_backward(_t(vals), _t(g), power=power, tile_rows=rows).cpu().numpy()
        print(f"[distortion] band 1-3, q={power}: dL_dvalues worst ratio {_check(got, ref, 'd_val', 'band'):.3e}")


def test_two_streams():
    import torch
    names = ("edge", "clamp")
    frames = [_frame(n) for n in names]
    inputs = [(_t(_values(f["scene"], f["cam"], "random")), _t(f["g"])) for f in frames]
    single = [f["r"].render_distortion(v, power=2).clone() for f, (v, g) in zip(frames, inputs)]
    moments = [f["r"]._distortion_moments[2] for f in frames]
    streams = [torch.cuda.Stream(device=DEV) for _ in frames]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for f, s, (v, g), m in zip(frames, streams, inputs, moments):
            with torch.cuda.stream(s):
                outs.append((f["r"].render_distortion(v, power=2, sync=False), f["r"].distortion_backward(v, g, power=2, moments=m, sync=False)))
    torch.cuda.synchronize()
    for i, (o, d) in enumerate(outs):
        assert torch.equal(o, single[i % 2])
        _check(d.cpu().numpy(), _walk(names[i % 2], "random", 2), "d_val", f"stream {i % 2}")


def test_nothing_rendered_writes_zeros():
    import torch
    scene, cam = SCENES["edge"]
    off = {k: v.copy() for k, v in scene.items()}
    off["means3D"][:, 0] += 500.0                            # every splat far off the frame: R == 0
    r = _rasterizer(off, cam)
    r.draw(cam)
    assert r.last_num_rendered == 0
    vals, g = _t(R.random_values(r.num_gaussians)), _t(R.gradient_of(cam))
    for power in R.POWERS:
        buf = torch.full((cam.height, cam.width), SENTINEL, dtype=torch.float32, device=DEV)
        r.render_distortion(vals, power=power, into=buf)
        assert (_bits(buf) == 0).all() and (_bits(r._distortion_moments[2]) == 0).all()
        assert (_bits(r.distortion_backward(vals, g, power=power)) == 0).all()
        res = r.backward(torch.zeros((3, cam.height, cam.width), device=DEV), distortion=(vals, g, power))
        assert (_bits(res["dL_dvalues"]) == 0).all() and (_bits(res["dL_dmean2D"]) == 0).all()
    r = _rasterizer(scene, cam)
    r.draw(cam, tile_rows=(1, 1))                            # an empty band: nothing is written
    buf = torch.full((cam.height, cam.width), SENTINEL, dtype=torch.float32, device=DEV)
    r.render_distortion(vals, tile_rows=(1, 1), into=buf)
    assert bool((buf == SENTINEL).all())
    assert (_bits(r.distortion_backward(vals, g, tile_rows=(1, 1))) == 0).all()


# ---- 2. the centring ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", R.POWERS)
def test_a_common_shift_of_1024_leaves_the_bits_of_out(power):
    """Values that are multiples of 2^-10 below 8, and the same values + 1024: every difference m - m0 is exact in both, so `out`
    is the same bit for bit — which holds only because the values are centred before they are squared."""
    for name in ("tile-257-faint", "edge"):
        f = _frame(name)
        r = f["r"]
        vals = (np.round(R.depth_values(f["scene"], f["cam"]) * 1024.0) / 1024.0).astype(np.float32)
        assert float(np.abs(vals).max()) < 8 and len(np.unique(vals)) > 20
        shifted = (vals + np.float32(1024.0)).astype(np.float32)
        assert np.array_equal((shifted.astype(np.float64) - 1024.0), vals.astype(np.float64))
        a, b = r.render_distortion(_t(vals), power=power).clone(), r.render_distortion(_t(shifted), power=power)
        assert float(a.abs().max()) > 0 and np.array_equal(_bits(a), _bits(b)), name
        # (the uncentred form would not: m^2 A - 2 m M1 + M2 at m = 1024 keeps no digit of a spread of 2^-10)


@pytest.mark.parametrize("power", R.POWERS)
def test_all_values_equal_give_exact_zeros(power):
    import torch
    f = _frame("edge")
    r, cam = f["r"], f["cam"]
    vals = torch.full((r.num_gaussians,), 3.7, dtype=torch.float32, device=DEV)
    out = r.render_distortion(vals, power=power)
    assert (_bits(out) == 0).all()
    res = r.backward(torch.zeros((3, cam.height, cam.width), device=DEV), distortion=(vals, _t(f["g"]), power), outputs=OUTPUTS)
    for k in OUTPUTS:
        assert (res[k] == 0).all(), (k, "the geometry sums the pass added are not exactly zero")
    if power == 2:          # (q = 1: the signed form's derivative 2 w (Ap - As) is not zero at equal values; it is checked against the reference)
        assert (res["dL_dvalues"] == 0).all()
    assert not bool(r._bw.scratch["sums_f64"].view(torch.int64).any()) and not bool(r._bw.scratch["distortion_sums_f64"].view(torch.int64).any())


# ---- 3. gradients ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", R.POWERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_value_and_geometry_gradients_within_the_bound(name, power):
    import torch
    f = _frame(name)
    r, cam = f["r"], f["cam"]
    n = r.num_gaussians
    zeros = torch.zeros((3, cam.height, cam.width), device=DEV)
    for kind in KINDS:
        vals, g = _t(_values(f["scene"], cam, kind)), _t(f["g"])
        fw, ref = _forward(name, kind, power), _walk(name, kind, power)
        r.render_distortion(vals, power=power)
        assert np.array_equal(_bits(r._distortion_moments[2]), _bits(fw["moments"]))
        # frozen geometry: dL_dvalues alone, sentinels around it, backward()'s scratch untouched
        r._bw.scratch.pop("sums_f64", None)
        buf = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device=DEV)
        r.distortion_backward(vals, g, power=power, into=buf[1:n + 1])
        host = buf.cpu().numpy()
        assert host[0] == SENTINEL and host[n + 1] == SENTINEL, "a write outside the output"
        assert "sums_f64" not in r._bw.scratch, "distortion_backward touched backward()'s scratch"
        assert not bool(r._bw.scratch["distortion_sums_f64"].view(torch.int64).any()), "the scratch is not left zero"
        _check(host[1:n + 1], ref, "d_val", f"{name} {kind} q={power} frozen")
        assert (_bits(host[1:n + 1][ref["pixels"] == 0]) == 0).all()
        # every geometry slot, through backward(distortion=...) with a zero colour gradient
        res = r.backward(zeros, distortion=(vals, g, power), outputs=OUTPUTS)
        _check_all(res, ref, f"{name} {kind} q={power}")
        assert (_bits(res["dL_dcolors"]) == 0).all(), "the colour slots are not this pass's"
        assert not bool(r._bw.scratch["sums_f64"].view(torch.int64).any()) and not bool(r._bw.scratch["distortion_sums_f64"].view(torch.int64).any())


def test_every_term_in_one_backward_call():
    """Colour + depth + opacity + features + distortion in one backward() against the sum of the references, each under its own
    bound (features_ref's with k, distortion_ref's with n); the scratches left zero; and gsr_backward's bits unchanged when no
    distortion is given."""
    import torch
    name, power, kind = "edge", 2, "depth"
    f = _frame(name)
    r, cam, st, scene = f["r"], f["cam"], f["st"], f["scene"]
    n, (H, W) = r.num_gaussians, (cam.height, cam.width)
    F, G = FR.features_of(n, 9), FR.gradient_of(cam, 9)
    gc, gd, ga = A.pixel_gradients(cam)
    d = A.depth_values(scene["means3D"], cam.view)
    chan, bg, g = FR.joint_channels(st["rgb"], r.background.cpu().numpy(), gc, F, G, d, gd, ga)
    ref_f = FR.backward(st, chan, bg, g, W, H)
    ref_d = _walk(name, kind, power)
    vals = _t(_values(scene, cam, kind))
    kw = dict(dL_ddepth=_t(gd), depth=True, dL_dalpha=_t(ga))
    plain = {k: v.clone() for k, v in r.backward(_t(gc), **kw).items()}
    r.render_distortion(vals, power=power)
    res = r.backward(_t(gc), features=(_t(F), _t(G)), distortion=(vals, _t(f["g"]), power), camera=True, **kw)
    worst = 0.0
    for out, key, part in GEO:
        got = res[out].cpu().numpy()[:, part].astype(np.float64)
        want, b = ref_f[key] + ref_d[key], FR.bound(ref_f, key) + R.bound(ref_d, key)
        assert (np.abs(got - want) <= b).all(), (key, float((np.abs(got - want) / b).max()))
        worst = max(worst, float((np.abs(got - want) / b).max()))
    print(f"[distortion] every term in one call: worst |err| / bound = {worst:.3e}")
    _check(res["dL_dvalues"].cpu().numpy(), ref_d, "d_val", "joint")
    part = {"d_chan": ref_f["d_chan"][:, 5:14], "M_d_chan": ref_f["M_d_chan"][:, 5:14], "k": ref_f["k"], "tiles": ref_f["tiles"]}
    assert (np.abs(res["dL_dfeatures"].cpu().numpy().astype(np.float64) - part["d_chan"]) <= FR.bound(part, "d_chan")).all()
    for k in ("sums_f64", "depth_sums_f64", "feature_sums_f64", "distortion_sums_f64"):
        assert not bool(r._bw.scratch[k].view(torch.int64).any()), k
    r.distortion_backward(vals, _t(f["g"]), power=power)
    again = r.backward(_t(gc), **kw)
    assert all(np.array_equal(_bits(plain[k]), _bits(again[k])) for k in plain), "gsr_backward's bits moved"


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------
def test_every_refusal_again_with_a_device_and_a_stale_receipt():
    import torch
    from gsrast_amd import _capi
    from test_distortion_cpu import REFUSALS, refused_untouched
    scene, cam = SCENES["edge"]
    r = _rasterizer(scene, cam)
    r.draw(cam)
    for case in REFUSALS:                                    # (decided before any HIP call: the addresses are never read)
        refused_untouched(case)
    n, (H, W) = r.num_gaussians, (cam.height, cam.width)
    zeros = torch.zeros((3, H, W), device=DEV)
    vals, g = _t(R.random_values(n)), _t(R.gradient_of(cam))
    with pytest.raises(AssertionError, match="stale"):       # no render_distortion yet
        r.distortion_backward(vals, g)
    with pytest.raises(AssertionError, match="power"):
        r.render_distortion(vals, power=3)
    r.render_distortion(vals, power=2)
    with pytest.raises(AssertionError, match="stale"):       # the moments are those of another power
        r.backward(zeros, distortion=(vals, g, 1))
    with pytest.raises(AssertionError, match="wide_sums"):
        r.backward(zeros, distortion=(vals, g), wide_sums=False)
    r.backward(zeros, distortion=(vals, g))
    r.draw(cam)                                              # another frame: the moments kept are stale
    with pytest.raises(AssertionError, match="stale"):
        r.backward(zeros, distortion=(vals, g))
    with pytest.raises(AssertionError, match="stale"):
        r.distortion_backward(vals, g)
    # a receipt of another size
    other = _rasterizer(*SCENES["fill"])
    other.draw(SCENES["fill"][1])
    with pytest.raises(_capi.GsrError) as e:
        r.render_distortion(vals, receipt=other.last_receipt)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG
    # a frame whose sorted lists were skipped: refused, the output untouched
    r.render_distortion(vals)
    moments = r._distortion_moments[2]
    r.draw(cam, plan="blocks", sorted_lists=False)
    assert r.last_plan == "blocks" and not r.last_lists_written
    out = torch.full((H, W), SENTINEL, dtype=torch.float32, device=DEV)
    with pytest.raises(_capi.GsrError) as e:
        r.render_distortion(vals, into=out)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG and bool((out == SENTINEL).all())
    with pytest.raises(_capi.GsrError):
        r.backward(zeros, distortion=(vals, g, 2, moments))
    assert "distortion_sums_f64" not in r._bw.scratch and "sums_f64" not in r._bw.scratch
    r.draw(cam)                                              # ... and the next frame is served again
    assert float(r.render_distortion(vals).abs().max()) > 0


# ---- 5. autograd -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_autograd_distortion_map(profile):
    import torch
    from gsrast_amd.autograd import FrameSlot, render
    from test_gpu_autograd import DRAW, RAW, _cam, _kw, _params, _rasterizer as _rast, _same_bits, _weights
    wt, wdt, _, _ = _weights()
    cam = _cam(1)
    n = _params(profile).num_gaussians
    V0 = _t(R.random_values(n))
    F0 = _t(FR.features_of(n, 5))
    # the tuple, with and without features=; a colour-only loss keeps its bits
    runs = {}
    for with_d in (False, True):
        params, rast = _params(profile), _rast()
        out = render(params, rast, cam, **_kw(profile), **DRAW, **({"distortion": V0} if with_d else {}))
        assert len(out) == (4 if with_d else 3)
        (wt * out[0]).sum().backward()
        runs[with_d] = (out[0].detach().clone(), [getattr(params, k).grad.clone() for k in RAW])
        if with_d:
            assert tuple(out[3].shape) == (rast.height, rast.width)
            assert np.array_equal(_bits(out[3]), _bits(rast.render_distortion(V0)))
    assert _same_bits(runs[False][0], runs[True][0]) and all(_same_bits(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    params, rast = _params(profile), _rast()
    out = render(params, rast, cam, features=F0, distortion=V0, distortion_power=1, **_kw(profile), **DRAW)
    assert len(out) == 5 and tuple(out[3].shape) == (5, rast.height, rast.width) and tuple(out[4].shape) == (rast.height, rast.width)
    assert np.array_equal(_bits(out[4]), _bits(rast.render_distortion(V0, power=1)))
    Gw = torch.rand((rast.height, rast.width), generator=torch.Generator().manual_seed(3)).to(DEV)
    # distortion="depth" with antialiasing and a FrameSlot: against the hand-run path, the gradient through z added by torch
    for aa in (False, True):
        params, rast, slot = _params(profile), _rast(), FrameSlot()
        color, dmap, omap, dist = render(params, rast, cam, depth=True, radii_slot=slot, antialiased=aa, distortion="depth", **_kw(profile), **DRAW)
        view = torch.from_numpy(np.asarray(cam.view, np.float32).reshape(-1)).to(DEV)
        m3 = rast.means3D.detach()
        z = (m3[:, 0] * view[2] + m3[:, 1] * view[6]) + (m3[:, 2] * view[10] + view[14])
        assert np.array_equal(_bits(dist), _bits(rast.render_distortion(z)))
        ((Gw * dist).sum() + (wdt * dmap).sum()).backward()
        zeros = torch.zeros_like(color)
        hand = rast.backward(zeros, semantics=profile, dL_ddepth=wdt, depth=True, distortion=(z, Gw),
                             outputs=("dL_dmean2D", "dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dconic_opacity"))
        assert _same_bits(slot.dL_dmean2D, hand["dL_dmean2D"])
        only_depth = rast.backward(zeros, semantics=profile, dL_ddepth=wdt, depth=True, outputs=("dL_dmean2D",))
        assert not _same_bits(only_depth["dL_dmean2D"], slot.dL_dmean2D)          # FrameSlot.dL_dmean2D holds the distortion term
        if not aa:
            # xyz: the chain's dL_dmeans3D plus dL_dvalues times row 2 of the view matrix (the activation copies xyz)
            want = hand["dL_dmeans3D"][:, :3] + hand["dL_dvalues"][:, None] * torch.stack([view[2], view[6], view[10]])[None, :]
            seen = slot.radii > 0
            got = params.xyz.grad
            assert bool((got[seen] != 0).any())
            assert bool((torch.abs(got - want)[seen] <= 1e-5 * torch.abs(want)[seen] + 1e-6 * float(want.abs().max())).all())
            assert bool((hand["dL_dvalues"] != 0).any())
        assert all(getattr(params, k).grad is not None and bool(torch.isfinite(getattr(params, k).grad).all()) for k in RAW[:4])
    # nothing but the values requires a gradient: the frozen-geometry pass
    params, rast = _params(profile, requires=()), _rast()
    V = V0.clone().requires_grad_(True)
    dist = render(params, rast, cam, distortion=V, **_kw(profile), **DRAW)[3]
    (Gw * dist).sum().backward()
    assert _same_bits(V.grad, rast.distortion_backward(V0, Gw)) and "sums_f64" not in rast._bw.scratch
    # a stale graph is refused
    params, rast = _params(profile), _rast()
    dist = render(params, rast, cam, distortion="depth", **_kw(profile), **DRAW)[3]
    render(params, rast, _cam(2), **_kw(profile), **DRAW)
    with pytest.raises(RuntimeError, match="has drawn another frame"):
        (Gw * dist).sum().backward()


def test_autograd_with_the_3d_filter_and_five_training_steps():
    """A two-layer scene: five Adam steps on the positions with the mean distortion as the only loss; it falls. The 3D filter
    stands between the parameters and the rasterizer and receives the term."""
    import torch
    from gsrast_amd.autograd import FrameSlot, GaussianParams, render
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer as _rast
    profile = "inria"
    cam, rast = _cam(1), _rast()
    raw = {k: np.array(v, copy=True) for k, v in _raw_scene(profile).items()}
    n = len(raw["xyz"])
    rng = np.random.default_rng(8)
    raw["xyz"][:, :2] = rng.uniform(-1.0, 1.0, (n, 2))
    raw["xyz"][:, 2] = np.where(np.arange(n) % 2 == 0, -0.4, 0.4) + rng.normal(0.0, 0.02, n)      # two layers
    params = GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major", device=DEV)
    filt = torch.full((n,), 0.01, dtype=torch.float32, device=DEV)
    opt = torch.optim.Adam([params.xyz], lr=2e-2)
    slot, losses = FrameSlot(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        dist = render(params, rast, cam, radii_slot=slot, distortion="depth", filter_3d=filt, **_kw(profile))[3]
        loss = dist.mean()
        losses.append(float(loss.detach()))
        loss.backward()
        assert bool(torch.isfinite(params.xyz.grad).all()) and bool((params.xyz.grad != 0).any())
        assert params.log_scale.grad is not None and bool((params.log_scale.grad != 0).any())      # (through the filter)
        opt.step()
    torch.cuda.synchronize()
    print(f"[distortion training] mean distortion {losses}")
    assert all(np.isfinite(losses)) and losses[0] > 0 and losses[-1] < losses[0]
