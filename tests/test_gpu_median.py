"""GPU: the median map and the per-pixel Gaussian ids of a drawn frame (include/gsrast_amd_median.h; SplatRasterizer.render_median,
.median_backward, .pick, autograd.rasterize / render(median=...), normals.normal_consistency(surface_depth=...)). The reference is
tests/median_ref.py's float32 restatement of the header over the forward state read back from the GPU: `out`, `ids` and
`dominant_ids` are compared with it bit for bit; tests/test_median_cpu.py establishes what that rests on (the replay's finalT /
nContrib are the oracle's bit for bit on every scene used here; the blindness guards). The backward is compared with the float64
sum: bit for bit where every sum is exact (g in multiples of 2^-10, |g| <= 1), else within
    |got - ref| <= ulp32(ref) + 2^-32 sum_{p -> i} |g(p)|
which is derived, not measured: at most 2^21 double additions, then one rounding."""
import functools

import numpy as np
import pytest

import median_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.0
ID_SENTINEL = 0x5A5A5A5A
SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
VARIANTS = {"sort": dict(plan="sort", deep_tiles=False), "blocks": dict(plan="blocks")}
NONE = int(R.NONE)


def _rasterizer(scene, cam):
    from gsrast_amd.rasterizer import SplatRasterizer
    r = SplatRasterizer(cam.width, cam.height, device=DEV)
    r.configure_from_scene(scene)
    return r


def _state(r):
    """The forward state of r's last draw(), as numpy arrays under the oracle's names."""
    g, im = r.map_geometry_state(), r.map_image_state()
    return {"means2D": g["means2D"].cpu().numpy(), "conicOpacity": g["conicOpacity"].cpu().numpy(),
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
    return R.depth_values(scene["means3D"], cam.view) if kind == "depth" else R.random_values(scene["means3D"].shape[0])


def _buffers(H, W):
    """(float [3,H,W], int [3,H,W], int [3,H,W]) full of sentinels: the calls write the middle planes."""
    import torch
    return (torch.full((3, H, W), SENTINEL, dtype=torch.float32, device=DEV),
            torch.full((3, H, W), ID_SENTINEL, dtype=torch.int32, device=DEV), torch.full((3, H, W), ID_SENTINEL, dtype=torch.int32, device=DEV))


def _untouched(bufs):
    f, i, d = (b.cpu().numpy() for b in bufs)
    return (f[0] == SENTINEL).all() and (f[2] == SENTINEL).all() and all((b[0] == ID_SENTINEL).all() and (b[2] == ID_SENTINEL).all() for b in (i, d))


@functools.lru_cache(maxsize=None)
def _frame(name):
    """One rasterizer per scene with its frame drawn and the state read back, computed once and left unchanged."""
    scene, cam = SCENES[name]
    r = _rasterizer(scene, cam)
    r.draw(cam, semantics="gscuda", sh_degree=0, plan="sort", tile_history=False)
    return dict(r=r, scene=scene, cam=cam, st=_state(r))


@functools.lru_cache(maxsize=None)
def _reference(name, threshold):
    f = _frame(name)
    ref = R.of_state(f["st"], f["cam"], None, threshold)
    assert np.array_equal(ref["nContrib"], f["st"]["nContrib"]) and np.array_equal(_bits(ref["finalT"]), _bits(f["st"]["finalT"])), name
    return ref


def _gather(ref, vals):
    out = np.zeros(ref["ids"].shape, np.float32)
    hit = ref["ids"] != R.NONE
    out[hit] = vals[ref["ids"][hit]]
    return out


# ---- 1. the three maps, bit for bit -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(SCENES))
def test_maps_bit_for_bit_against_the_restatement(name, variant, semantics):
    import ctypes as C
    import torch
    from gsrast_amd import _capi
    from gsrast_amd.contrib import contribution_args
    scene, cam = SCENES[name]
    H, W = cam.height, cam.width
    r = _rasterizer(scene, cam)
    r.draw(cam, semantics=semantics, sh_degree=0, tile_history=False, **VARIANTS[variant])
    assert r.last_plan == VARIANTS[variant]["plan"] and r.last_lists_written, (name, r.last_plan)
    st = _state(r)
    before = _chunks(r)
    values = {kind: _values(scene, cam, kind) for kind in ("depth", "random")}
    for threshold in R.THRESHOLDS:
        ref = R.of_state(st, cam, None, threshold, semantics)
        assert np.array_equal(ref["nContrib"], st["nContrib"]) and np.array_equal(_bits(ref["finalT"]), _bits(st["finalT"])), (name, variant, semantics)
        for kind, vals in values.items():
            bufs = _buffers(H, W)
            res = r.render_median(_t(vals), threshold=threshold, ids=True, dominant=True,
                                  out={"map": bufs[0][1], "ids": bufs[1][1], "dominant_ids": bufs[2][1]})
            assert res["map"].data_ptr() == bufs[0][1].data_ptr() and _untouched(bufs), "a write outside the outputs"
            what = (name, variant, semantics, threshold, kind)
            assert np.array_equal(_bits(res["ids"]), ref["ids"]), what + ("ids",)
            assert np.array_equal(_bits(res["dominant_ids"]), ref["dominant_ids"]), what + ("dominant_ids",)
            assert np.array_equal(_bits(res["map"]), _bits(_gather(ref, vals))), what + ("out",)
        if threshold == 0.0:
            # on the device's own arrays: the last blended record is the forward's last contributor
            ids = _bits(res["ids"])
            ys, xs = np.nonzero(st["nContrib"] > 0)
            tile = (ys // 16) * ((W + 15) // 16) + xs // 16
            ranges = st["ranges"].reshape(-1, 2).astype(np.int64)
            assert np.array_equal(ids[ys, xs], st["values"][ranges[tile, 0] + st["nContrib"][ys, xs].astype(np.int64) - 1])
            assert (ids[st["nContrib"] == 0] == NONE).all()
    # the histogram of dominant_ids is gsr_contribution's `dominant`
    dominant = torch.zeros((r.num_gaussians,), dtype=torch.int64, device=DEV)
    a = contribution_args(r, r.last_receipt, semantics, {"dominant": dominant.data_ptr()})
    _capi.call("gsr_contribution", C.byref(a), device=r.device)
    torch.cuda.synchronize()
    dom = _bits(res["dominant_ids"])
    hist = np.bincount(dom[dom != NONE].astype(np.int64), minlength=r.num_gaussians)
    assert np.array_equal(hist, dominant.cpu().numpy()), (name, variant, semantics)
    after = _chunks(r)
    assert len(before) == len(after) and all(torch.equal(a, b) for a, b in zip(before, after)), "a chunk was written"


@pytest.mark.parametrize("name", ["tile-600-opaque", "edge", "fill"])
def test_each_output_alone(name):
    f = _frame(name)
    r, cam = f["r"], f["cam"]
    vals = _values(f["scene"], cam, "random")
    for threshold in R.THRESHOLDS:
        ref = _reference(name, threshold)
        only = r.render_median(_t(vals), threshold=threshold, ids=False)
        assert set(only) == {"map"} and np.array_equal(_bits(only["map"]), _bits(_gather(ref, vals)))
        only = r.render_median(threshold=threshold)
        assert set(only) == {"ids"} and np.array_equal(_bits(only["ids"]), ref["ids"])
        only = r.render_median(threshold=threshold, ids=False, dominant=True)
        assert set(only) == {"dominant_ids"} and np.array_equal(_bits(only["dominant_ids"]), ref["dominant_ids"])
    with pytest.raises(AssertionError, match="nothing asked for"):
        r.render_median(ids=False)


def test_bands_of_tile_rows_leave_the_other_rows_alone():
    import torch
    f = _frame("fill")
    r, cam = f["r"], f["cam"]
    H, W = cam.height, cam.width
    vals = _values(f["scene"], cam, "depth")
    ref = _reference("fill", 0.5)
    want = {"map": _bits(_gather(ref, vals)), "ids": ref["ids"], "dominant_ids": ref["dominant_ids"]}
    # any band inside the rows the draw() covered
    for rows in ((1, 3), (0, 1), (7, 8), (0, 8)):
        y0, y1 = 16 * rows[0], 16 * rows[1]
        bufs = _buffers(H, W)
        res = r.render_median(_t(vals), dominant=True, tile_rows=rows, out={"map": bufs[0][1], "ids": bufs[1][1], "dominant_ids": bufs[2][1]})
        assert _untouched(bufs)
        for k, sentinel in (("map", _bits(np.float32(SENTINEL))), ("ids", ID_SENTINEL), ("dominant_ids", ID_SENTINEL)):
            got = _bits(res[k])
            assert np.array_equal(got[y0:y1], want[k][y0:y1]), (rows, k)
            assert (got[:y0] == sentinel).all() and (got[y1:] == sentinel).all(), (rows, k, "a row outside the band was written")
    new = r.render_median(_t(vals), tile_rows=(2, 3))          # new tensors: 0 / -1 outside the band
    assert (new["map"][:32] == 0).all() and (new["ids"][48:] == -1).all() and np.array_equal(_bits(new["ids"][32:48]), want["ids"][32:48])
    # a frame drawn as a band: its own rows by default, rows outside them refused
    from gsrast_amd import _capi
    scene = f["scene"]
    r2 = _rasterizer(scene, cam)
    r2.draw(cam, tile_rows=(1, 3), plan="sort", tile_history=False)
    st = _state(r2)
    ref2 = R.of_state(st, cam, None, 0.5, tile_rows=(1, 3))
    buf = torch.full((H, W), ID_SENTINEL, dtype=torch.int32, device=DEV)
    r2.render_median(out={"ids": buf})
    got = _bits(buf)
    assert np.array_equal(got[16:48], ref2["ids"][16:48]) and (got[:16] == ID_SENTINEL).all() and (got[48:] == ID_SENTINEL).all()
    with pytest.raises(_capi.GsrError) as e:
        r2.render_median(tile_rows=(0, 3), out={"ids": buf})
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG and np.array_equal(_bits(buf), got)


def test_two_streams():
    import torch
    names = ("edge", "tile-257-opaque")
    frames = [_frame(n) for n in names]
    inputs = [(_t(_values(f["scene"], f["cam"], "random")), _t(R.exact_gradient(f["cam"]))) for f in frames]
    single = []
    for f, (v, g) in zip(frames, inputs):
        res = f["r"].render_median(v, dominant=True)
        single.append((res, f["r"].median_backward(res["ids"], g).clone()))
    streams = [torch.cuda.Stream(device=DEV) for _ in frames]
    torch.cuda.synchronize()
    outs = []
    for _ in range(3):
        for f, s, (v, g) in zip(frames, streams, inputs):
            with torch.cuda.stream(s):
                res = f["r"].render_median(v, dominant=True, sync=False)
                outs.append((res, f["r"].median_backward(res["ids"], g, sync=False)))
    torch.cuda.synchronize()
    for i, (res, d) in enumerate(outs):
        want, dwant = single[i % 2]
        assert all(torch.equal(res[k], want[k]) for k in want) and np.array_equal(_bits(d), _bits(dwant))


def test_nothing_rendered_gives_zeros_and_none():
    import torch
    scene, cam = SCENES["edge"]
    H, W = cam.height, cam.width
    off = {k: v.copy() for k, v in scene.items()}
    off["means3D"][:, 0] += 500.0                            # every splat far off the frame: R == 0
    r = _rasterizer(off, cam)
    r.draw(cam)
    assert r.last_num_rendered == 0
    vals = _t(R.random_values(r.num_gaussians))
    bufs = _buffers(H, W)
    res = r.render_median(vals, dominant=True, out={"map": bufs[0][1], "ids": bufs[1][1], "dominant_ids": bufs[2][1]})
    assert _untouched(bufs) and (_bits(res["map"]) == 0).all() and (_bits(res["ids"]) == NONE).all() and (_bits(res["dominant_ids"]) == NONE).all()
    assert (_bits(r.median_backward(res["ids"], _t(R.random_gradient(cam)))) == 0).all()
    assert r.pick(5, 5) is None and r.pick(5, 5, dominant=True) is None
    r = _rasterizer(scene, cam)
    r.draw(cam, tile_rows=(1, 1))                            # an empty band: nothing is written
    bufs = _buffers(H, W)
    r.render_median(vals, dominant=True, out={"map": bufs[0][1], "ids": bufs[1][1], "dominant_ids": bufs[2][1]})
    assert _untouched(bufs) and bool((bufs[0][1] == SENTINEL).all()) and bool((bufs[1][1] == ID_SENTINEL).all()) and bool((bufs[2][1] == ID_SENTINEL).all())
    ids = torch.zeros((H, W), dtype=torch.int32, device=DEV)
    assert (_bits(r.median_backward(ids, _t(R.random_gradient(cam)), tile_rows=(1, 1))) == 0).all()


# ---- 2. the backward --------------------------------------------------------------------------------------------------------------
def _backward(r, ids, g, n, **kw):
    """median_backward into a tensor with a sentinel at either end; the scratch left zero."""
    import torch
    buf = torch.full((n + 2,), SENTINEL, dtype=torch.float32, device=DEV)
    got = r.median_backward(ids, g, into=buf[1:n + 1], **kw)
    host = buf.cpu().numpy()
    assert got.data_ptr() == buf[1:].data_ptr() and host[0] == SENTINEL and host[n + 1] == SENTINEL, "a write outside the output"
    assert not bool(r._bw.scratch["median_sums_f64"].view(torch.int64).any()), "the scratch is not left zero"
    return host[1:n + 1].copy()


@pytest.mark.parametrize("name", list(SCENES))
def test_backward_exact_and_within_the_bound(name):
    f = _frame(name)
    r, cam = f["r"], f["cam"]
    n = r.num_gaussians
    for threshold in (0.5, R.FIRST_HIT):
        ref = _reference(name, threshold)
        ids = r.render_median(threshold=threshold)["ids"]
        assert np.array_equal(_bits(ids), ref["ids"])
        # every sum exact: bit for bit, twice
        g = R.exact_gradient(cam)
        sums, mags, pixels = R.backward(ref["ids"], g, n)
        got = _backward(r, ids, _t(g), n)
        assert np.array_equal(_bits(got), _bits(sums.astype(np.float32))), (name, threshold, "exact")
        assert (_bits(got[pixels == 0]) == 0).all(), "a row nothing selected must be +0.0"
        assert np.array_equal(_bits(_backward(r, ids, _t(g), n)), _bits(got)), "two calls differ"
        if name == "fill" and threshold == R.FIRST_HIT:
            tiles = {(y // 16, x // 16) for y, x in zip(*np.nonzero(ref["ids"] == 0))}
            assert len(tiles) == 64 and pixels[0] > 6400, "the screen-filling Gaussian is the first hit of every tile"
        # random g: the derived bound
        g = R.random_gradient(cam)
        sums, mags, pixels = R.backward(ref["ids"], g, n)
        got = _backward(r, ids, _t(g), n).astype(np.float64)
        err, bound = np.abs(got - sums), R.backward_bound(sums, mags)
        print(f"[median backward] {name} threshold {threshold:g}: worst |err| / bound {float((err / bound).max()):.3e}, "
              f"most pixels a row {int(pixels.max())}")
        assert (err <= bound).all(), (name, threshold, float((err / bound).max()))
        assert (_bits(got.astype(np.float32)[pixels == 0]) == 0).all()


def test_backward_drops_ids_that_name_no_gaussian_and_bands():
    import torch
    f = _frame("fill")
    r, cam = f["r"], f["cam"]
    n = r.num_gaussians
    ref = _reference("fill", 0.5)
    ids = ref["ids"].copy()
    rng = np.random.default_rng(3)
    ys, xs = rng.integers(0, cam.height, 600), rng.integers(0, cam.width, 600)
    ids[ys[:200], xs[:200]] = n                              # the first id that names nobody
    ids[ys[200:400], xs[200:400]] = n + 12345
    ids[ys[400:], xs[400:]] = R.NONE
    g = R.exact_gradient(cam)
    sums, _, pixels = R.backward(ids, g, n)
    dev_ids = _t(ids.view(np.int32))
    got = _backward(r, dev_ids, _t(g), n)
    assert np.array_equal(_bits(got), _bits(sums.astype(np.float32))) and (_bits(got[pixels == 0]) == 0).all()
    for rows in ((1, 3), (7, 8), (2, 2)):
        sums, _, _ = R.backward(ids, g, n, tile_rows=rows)
        assert np.array_equal(_bits(_backward(r, dev_ids, _t(g), n, tile_rows=rows)), _bits(sums.astype(np.float32))), rows
    # one id everywhere: 64 tiles, four strips each, into one row
    one = torch.full((cam.height, cam.width), 7, dtype=torch.int32, device=DEV)
    got = _backward(r, one, _t(g), n)
    assert got[7] == np.float32(g.astype(np.float64).sum()) and (_bits(np.delete(got, 7)) == 0).all()


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_every_refusal_again_with_a_device_and_the_python_layer():
    import torch
    from gsrast_amd import _capi
    from test_median_cpu import REFUSALS, refused_untouched
    scene, cam = SCENES["edge"]
    H, W = cam.height, cam.width
    r = _rasterizer(scene, cam)
    r.draw(cam)
    for case in REFUSALS:                                    # (decided before any HIP call: the addresses are never read)
        refused_untouched(case)
    n = r.num_gaussians
    vals, g = _t(R.random_values(n)), _t(R.exact_gradient(cam))
    buf = torch.full((H, W), ID_SENTINEL, dtype=torch.int32, device=DEV)
    for threshold in (1.0, -0.25, float("nan")):
        with pytest.raises(_capi.GsrError) as e:
            r.render_median(vals, threshold=threshold, out={"ids": buf})
        assert e.value.code == _capi.GSR_ERR_INVALID_ARG and bool((buf == ID_SENTINEL).all())
    other = _rasterizer(*SCENES["fill"])                     # a receipt of another size
    other.draw(SCENES["fill"][1])
    with pytest.raises(_capi.GsrError) as e:
        r.render_median(vals, receipt=other.last_receipt)
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG
    ids = r.render_median(vals)["ids"]
    want = r.median_backward(ids, g).clone()
    # a frame whose sorted lists were skipped: the forward is refused, the outputs untouched ...
    r.draw(cam, plan="blocks", sorted_lists=False)
    assert r.last_plan == "blocks" and not r.last_lists_written
    with pytest.raises(_capi.GsrError) as e:
        r.render_median(vals, out={"ids": buf})
    assert e.value.code == _capi.GSR_ERR_INVALID_ARG and bool((buf == ID_SENTINEL).all())
    with pytest.raises(_capi.GsrError):
        r.pick(20, 12)
    # ... and the backward, which reads nothing of the frame, gives the same bits as before
    assert np.array_equal(_bits(r.median_backward(ids, g)), _bits(want))
    r.draw(cam)                                              # the next frame is served again
    assert bool((r.render_median(vals)["ids"] >= 0).any())


# ---- 4. pick ------------------------------------------------------------------------------------------------------------------------
def test_pick_is_the_maps_entry_and_walks_one_tile_row():
    f = _frame("fill")
    r, cam = f["r"], f["cam"]
    full = {t: r.render_median(threshold=t, dominant=True) for t in (0.5, R.FIRST_HIT)}
    rng = np.random.default_rng(11)
    calls = []
    inner = r.render_median

    def spy(*args, **kw):
        res = inner(*args, **kw)
        calls.append((kw, res))
        return res
    r.render_median = spy
    try:
        points = [(0, 0), (cam.width - 1, cam.height - 1), (17, 15), (17, 16)] + [(int(rng.integers(cam.width)), int(rng.integers(cam.height))) for _ in range(12)]
        for x, y in points:
            for t in full:
                for dominant in (False, True):
                    want = int(full[t]["dominant_ids" if dominant else "ids"][y, x])
                    assert r.pick(x, y, threshold=t, dominant=dominant) == (None if want < 0 else want), (x, y, t, dominant)
                    kw, res = calls[-1]
                    row = y // 16
                    assert kw["tile_rows"] == (row, row + 1) and len(res) == 1
                    (k, m), = res.items()
                    m = m.cpu().numpy()
                    assert (m[:16 * row] == -1).all() and (m[16 * row + 16:] == -1).all(), "a row outside the pixel's tile row was walked"
                    assert np.array_equal(m[16 * row:16 * row + 16], full[t][k].cpu().numpy()[16 * row:16 * row + 16])
    finally:
        del r.render_median
    assert any(r.pick(x, y) is not None for x, y in points)
    edge = _frame("edge")["r"]                               # (its columns 0 and 1 are out of every splat's reach)
    assert edge.pick(0, 5) is None and edge.pick(1, 20, dominant=True) is None and edge.pick(20, 12) is not None
    with pytest.raises(AssertionError):
        r.pick(cam.width, 0)


# ---- 5. autograd --------------------------------------------------------------------------------------------------------------------
def _autograd_helpers():
    import test_gpu_autograd as T
    return T


@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_autograd_median_depth(profile):
    import torch
    from gsrast_amd import autograd
    T = _autograd_helpers()
    wt, wdt, _, _ = T._weights()
    cam = T._cam(1)
    kw = dict(**T._kw(profile), **T.DRAW)
    Gw = torch.rand((T.H, T.W), generator=torch.Generator().manual_seed(5)).to(DEV) - 0.25
    # median=None: image and gradients are what they are without the argument; with it, a colour-only loss keeps its bits
    runs = {}
    for with_m in (False, True):
        params, rast = T._params(profile), T._rasterizer()
        out = autograd.render(params, rast, cam, **kw, **({"median": "depth"} if with_m else {"median": None}))
        assert len(out) == (4 if with_m else 3)
        (wt * out[0]).sum().backward()
        runs[with_m] = (out[0].detach().clone(), [getattr(params, k).grad.clone() for k in T.RAW])
    assert T._same_bits(runs[False][0], runs[True][0]) and all(T._same_bits(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    # the map has the plain call's bits; its gradients against the float64 composition fed the call's own ids
    for threshold in (0.5, 0.05):
        params, rast, slot = T._params(profile), T._rasterizer(), autograd.RadiiSlot()
        view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, rast.device)
        view = view.clone().requires_grad_(True)
        out = autograd.render(params, rast, (view, proj, cam_pos, tx, ty), radii_slot=slot, median="depth", median_threshold=threshold, **kw)
        med = out[3]
        assert tuple(med.shape) == (T.H, T.W) and med.requires_grad
        m3 = rast.means3D.detach()
        v = view.detach().reshape(-1)
        z = (m3[:, 0] * v[2] + m3[:, 1] * v[6]) + (m3[:, 2] * v[10] + v[14])
        plain = rast.render_median(z, threshold=threshold)
        assert T._same_bits(med, plain["map"]) and bool((plain["ids"] >= 0).any()) and bool((plain["ids"] < 0).any())
        ids = plain["ids"].cpu().numpy().view(np.uint32)
        # the backward succeeds after the rasterizer has drawn again: it holds the id map and nothing of the frame
        autograd.render(T._params(profile), rast, T._cam(2), **kw)
        (Gw * med).sum().backward()
        d_m, d_v = R.depth_gradients64(m3.cpu().numpy(), v.cpu().numpy(), ids, Gw.cpu().numpy())
        want = torch.from_numpy(d_m[:, :3]).to(DEV)
        got = params.xyz.grad.double()
        seen = slot.radii > 0
        assert bool((got[seen] != 0).any()) and bool((got[~seen] == 0).all())
        assert bool((torch.abs(got - want)[seen] <= 1e-5 * torch.abs(want)[seen] + 1e-6 * float(want.abs().max())).all()), threshold
        want_v = torch.from_numpy(d_v).to(DEV)
        got_v = view.grad.double().reshape(-1)
        assert bool((torch.abs(got_v - want_v) <= 1e-5 * torch.abs(want_v) + 1e-6 * float(want_v.abs().max())).all()), threshold
        assert bool((got_v[[2, 6, 10, 14]] != 0).all()) and bool((np.delete(got_v.cpu().numpy(), [2, 6, 10, 14]) == 0).all())
        # what is not differentiated: nothing reaches the shape or the opacity through the map
        assert all(getattr(params, k).grad is None or not bool(getattr(params, k).grad.any()) for k in ("log_scale", "rotation", "opacity_logit"))
    # a tensor of the caller's: the frozen selection's gradient is median_backward's
    params, rast = T._params(profile, requires=()), T._rasterizer()
    V = _t(R.random_values(params.num_gaussians)).requires_grad_(True)
    med = autograd.render(params, rast, cam, median=V, **kw)[3]
    (Gw * med).sum().backward()
    ids = rast.render_median()["ids"]
    assert T._same_bits(V.grad, rast.median_backward(ids, Gw)) and bool((V.grad != 0).any())
    with pytest.raises(ValueError, match="median"):
        autograd.render(params, rast, cam, median=V[:-1], **kw)
    with pytest.raises(ValueError, match="median_threshold"):
        autograd.render(params, rast, cam, median="depth", median_threshold=1.0, **kw)


def test_the_tuples_order_with_every_other_option():
    import torch
    from gsrast_amd import autograd
    T = _autograd_helpers()
    profile = "inria"
    cam = T._cam(1)
    n = T._params(profile).num_gaussians
    F0 = torch.rand((n, 5), generator=torch.Generator().manual_seed(2)).to(DEV)
    filt = torch.full((n,), 0.01, dtype=torch.float32, device=DEV)
    params, rast = T._params(profile), T._rasterizer()
    out = autograd.render(params, rast, cam, depth=True, opacity_grad=True, antialiased=True, filter_3d=filt, features=F0, normals=True,
                          distortion="depth", median="depth", **T._kw(profile), **T.DRAW)
    shapes = [None if t is None else tuple(t.shape) for t in out]
    assert shapes == [(3, T.H, T.W), (T.H, T.W), (T.H, T.W), (5, T.H, T.W), (3, T.H, T.W), (T.H, T.W), (T.H, T.W)], shapes
    m3 = rast.means3D.detach()
    v = autograd._camera_tensors(cam, rast.device)[0].reshape(-1)
    z = (m3[:, 0] * v[2] + m3[:, 1] * v[6]) + (m3[:, 2] * v[10] + v[14])
    assert T._same_bits(out[6], rast.render_median(z)["map"]) and T._same_bits(out[5], rast.render_distortion(z))
    assert not T._same_bits(out[6], out[5])
    loss = sum(t.mean() for t in out)
    loss.backward()
    assert all(bool(torch.isfinite(getattr(params, k).grad).all()) for k in T.RAW)
    # each alone behind the three
    for extra, length in ((dict(), 4), (dict(features=F0), 5), (dict(normals=True), 5), (dict(distortion="depth"), 5)):
        out = autograd.render(T._params(profile), rast, cam, median="depth", **extra, **T._kw(profile), **T.DRAW)
        assert len(out) == length and tuple(out[-1].shape) == (T.H, T.W) and T._same_bits(out[-1], rast.render_median(z)["map"])


def test_five_training_steps_with_the_median_depth_as_the_surface():
    import torch
    from gsrast_amd import autograd, normals
    from gsrast_amd.optim import GaussianAdam
    T = _autograd_helpers()
    profile = "inria"
    cam, rast = T._cam(1), T._rasterizer()
    tan = (float(cam.tan_fovx), float(cam.tan_fovy))
    raw = {k: v.copy() for k, v in T._raw_scene(profile).items()}
    raw["log_scale"][:, 2] -= np.float32(np.log(12.0))
    params = autograd.GaussianParams.from_raw(*(raw[k] for k in T.RAW), sh_layout="coefficient_major", device=DEV)
    rates = {"xyz": 1e-3, "opacity_logit": 1e-2, "log_scale": 5e-3, "rotation": 2e-2, "shs": 1e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    slot, losses = autograd.RadiiSlot(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        color, dmap, omap, nmap, med = autograd.render(params, rast, cam, depth=True, opacity_grad=True, normals=True, median="depth",
                                                       radii_slot=slot, **T._kw(profile))
        cons = normals.normal_consistency(nmap, None, omap, tan, semantics=profile, surface_depth=med)
        default = normals.normal_consistency(nmap, dmap, omap, tan, semantics=profile)
        assert tuple(cons.shape) == (T.H, T.W) and not T._same_bits(cons, default)
        loss = cons.mean()
        losses.append(float(loss.detach()))
        loss.backward()
        for k in T.RAW[:4]:
            grad = getattr(params, k).grad
            assert bool(torch.isfinite(grad).all()) and bool((grad[slot.radii <= 0] == 0).all()), k
        assert bool((params.rotation.grad != 0).any()) and bool((params.xyz.grad != 0).any())
        opt.step(slot.radii)
    torch.cuda.synchronize()
    print(f"[median] normal consistency on the median depth over five steps: {' '.join(f'{v:.6f}' for v in losses)}")
    assert all(np.isfinite(losses))
