"""GPU: antialiased splatting (include/gsrast_amd_antialias.h, gsrast_amd/antialias.py, rasterize / render with
antialiased=True). The forward bit for bit against the float32 restatement of tests/antialias_ref.py, the backward against
its float64 autograd function within BOUNDS, and the composition with the rasterizer: image bits, raw-parameter gradients,
the default path untouched, a short training run. The scenes' own preconditions are tests/test_antialias_cpu.py's."""
import ctypes as C
import functools

import numpy as np
import pytest

import activation_ref as A
import antialias_ref as R

pytestmark = pytest.mark.gpu

PROFILES = ("gscuda", "inria")
PAD = 64                        # floats of sentinel on each side of every array written (256 bytes: the rows stay 16-byte aligned)
SENTINEL = -777.25


def _torch():
    import torch
    return torch


def _dev(a, dtype=np.float32):
    return _torch().from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _bits(t):
    torch = _torch()
    t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t))
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


class _Guarded:
    """A device array of `floats` floats between two runs of sentinels."""

    def __init__(self, floats):
        self.buf = _torch().full((floats + 2 * PAD,), SENTINEL, dtype=_torch().float32, device="cuda")
        self.floats = floats

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def inner(self):
        return self.buf[PAD:PAD + self.floats]

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.floats:] == SENTINEL).all())


def _inputs(scene, cam):
    t = {k: _dev(scene[k]) for k in ("means3D", "scales", "rotations", "opacities")}
    t["view"], t["proj"] = _dev(cam.view), _dev(cam.proj)
    return t


def _fill(a, t, n, cam, semantics, scale_modifier, stream):
    from gsrast_amd import _capi
    a.struct_size = C.sizeof(type(a))
    a.flags = _capi.GSR_FLAG_SEMANTICS_INRIA if semantics == "inria" else 0
    a.num_gaussians, a.width, a.height = n, cam.width, cam.height
    a.tan_fovx, a.tan_fovy, a.scale_modifier = cam.tan_fovx, cam.tan_fovy, scale_modifier
    a.means3D, a.scales, a.rotations, a.opacities = (t[k].data_ptr() for k in ("means3D", "scales", "rotations", "opacities"))
    a.view_matrix = t["view"].data_ptr()
    a.proj_matrix = t["proj"].data_ptr() if semantics == "gscuda" else None      # (the upstream profile does not read it)
    a.stream = stream if stream is not None else _torch().cuda.current_stream().cuda_stream


def _forward(t, n, cam, semantics, scale_modifier=1.0, outputs=("o", "c"), stream=None):
    """The plain C call into guarded arrays: {"o": o', "c": c} (device tensors), after checking the sentinels."""
    from gsrast_amd import _capi
    out = {k: _Guarded(n) for k in outputs}
    a = _capi.AntialiasArgs()
    _fill(a, t, n, cam, semantics, scale_modifier, stream)
    a.opacities_out = out["o"].ptr if "o" in out else None
    a.compensation = out["c"].ptr if "c" in out else None
    _capi.call("gsr_antialias_forward", C.byref(a))
    _torch().cuda.synchronize()
    assert all(g.intact() for g in out.values()), "a write outside an output array"
    return {k: g.inner() for k, g in out.items()}


BACKWARD_OUTPUTS = {"opacities": 1, "means3D": 4, "scales": 4, "rotations": 4}


def _backward(t, n, cam, semantics, g, radii, scale_modifier=1.0, outputs=tuple(BACKWARD_OUTPUTS)):
    from gsrast_amd import _capi
    out = {k: _Guarded(n * BACKWARD_OUTPUTS[k]) for k in outputs}
    a = _capi.AntialiasBackwardArgs()
    _fill(a, t, n, cam, semantics, scale_modifier, None)
    a.dL_dopacities_out = g.data_ptr()
    a.radii = radii.data_ptr() if radii is not None else None
    p = lambda k: out[k].ptr if k in out else None
    a.dL_dopacities, a.dL_dmeans3D, a.dL_dscales, a.dL_drotations = p("opacities"), p("means3D"), p("scales"), p("rotations")
    _capi.call("gsr_antialias_backward", C.byref(a))
    _torch().cuda.synchronize()
    assert all(gd.intact() for gd in out.values()), "a write outside an output array"
    return {k: gd.inner().reshape(n, BACKWARD_OUTPUTS[k]) if BACKWARD_OUTPUTS[k] > 1 else gd.inner() for k, gd in out.items()}


# ---- forward ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", PROFILES)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_forward_is_the_float32_restatement_bit_for_bit(n, semantics):
    """The needle scene (needles, splats far below a pixel, behind the camera, beyond the +-1.3 clamp, scales of 0, 1e9 and
    3e18, a zero quaternion; non-square pixels under the upstream profile) at scale_modifier 1, 0.5 and 2, and the
    conditioned scene; each output alone; on a second stream."""
    torch = _torch()
    cam = R.camera(semantics)
    for scene in (R.first_rows(R.needle_scene(semantics), n), R.first_rows(R.conditioned_scene(semantics), n)):
        t = _inputs(scene, cam)
        before = {k: v.clone() for k, v in t.items()}
        for mod in (1.0, 0.5, 2.0):
            want = R.compensation_f32(scene["means3D"], scene["scales"], scene["rotations"], scene["opacities"], cam.view, cam.proj,
                                      cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, semantics, mod)
            got = _forward(t, n, cam, semantics, mod)
            assert _same_bits(got["c"], want["c"]), (n, semantics, mod, int((_bits(got["c"]) != _bits(want["c"])).sum()))
            assert _same_bits(got["o"], want["o_out"]), (n, semantics, mod)
            dead = want["culled"] | want["d1_bad"]
            assert (got["c"].cpu().numpy()[dead] == 1.0).all()
        only_c, only_o = _forward(t, n, cam, semantics, 2.0, outputs=("c",)), _forward(t, n, cam, semantics, 2.0, outputs=("o",))
        assert _same_bits(only_c["c"], got["c"]) and _same_bits(only_o["o"], got["o"])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        other = _forward(t, n, cam, semantics, 2.0, stream=side.cuda_stream)
        assert _same_bits(other["c"], got["c"]) and _same_bits(other["o"], got["o"])
        assert all(_same_bits(before[k], t[k]) for k in t), "an input was written"
    if n == 1000:
        live = ~(want["culled"] | want["d1_bad"])
        assert dead.any() and want["floored"].any() and (want["c"][live] < 0.5).any() and (want["c"][live] > 0.99).any()


def test_python_compensation_returns_the_calls_outputs():
    from gsrast_amd import antialias
    for semantics in PROFILES:
        cam, scene = R.camera(semantics), R.first_rows(R.conditioned_scene(semantics), 300)
        t = _inputs(scene, cam)
        want = R.masks_of(scene, cam, semantics)
        o, c = antialias.compensation(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["view"], (cam.tan_fovx, cam.tan_fovy),
                                      cam.width, cam.height, semantics=semantics, proj=t["proj"] if semantics == "gscuda" else None)
        assert _same_bits(o, want["o_out"]) and _same_bits(c, want["c"])
    with pytest.raises(ValueError):
        antialias.compensation(t["means3D"], t["scales"], t["rotations"], t["opacities"], t["view"], (0.4, 0.4), 64, 48, semantics="gscuda")


# ---- backward ---------------------------------------------------------------------------------------------------------------------
def _backward_case(semantics, n=None):
    """The conditioned scene with its seeded dL/do' and radii (a sixth of them <= 0); five rows whose g is zero get NaN inputs."""
    scene = dict(R.conditioned_scene(semantics))
    if n is not None:
        scene = R.first_rows(scene, n)
    scene = {k: v.copy() for k, v in scene.items()}
    n = scene["opacities"].shape[0]
    g = R.seed_gradient(n)
    rng = np.random.default_rng(77)
    radii = rng.integers(1, 40, n).astype(np.int32)
    off = rng.uniform(size=n) < 1.0 / 6.0
    radii[off] = np.where(rng.uniform(size=off.sum()) < 0.5, 0, -1)
    poisoned = np.nonzero((g == 0) & (radii > 0))[0][:5]
    scene["means3D"][poisoned, :3] = np.nan
    scene["scales"][poisoned[:3], :3] = np.nan
    scene["rotations"][poisoned[3:], :] = np.nan
    return scene, g, radii, poisoned


@pytest.mark.parametrize("semantics", PROFILES)
def test_backward_matches_the_float64_reference(semantics):
    cam = R.camera(semantics)
    scene, g, radii, poisoned = _backward_case(semantics)
    n = len(g)
    assert len(poisoned) == 5
    t = _inputs(scene, cam)
    before = {k: v.clone() for k, v in t.items()}
    got = {k: v.cpu().numpy() for k, v in _backward(t, n, cam, semantics, _dev(g), _dev(radii, np.int32)).items()}
    masks = R.masks_of(scene, cam, semantics)
    on = (radii > 0) & (g != 0)
    # dL/do = c g: one product, bit for bit; +0 in the rows that are off
    want_o = np.where(on, masks["c"] * g, np.float32(0.0)).astype(np.float32)
    assert np.array_equal(got["opacities"].view(np.uint32), want_o.view(np.uint32))
    # exact +0 zeros: culled by the frame, no gradient, floored, culled by the profile, d1 zero or not finite
    zero = ~on | ~masks["flows"]
    assert (masks["floored"] & on).sum() >= 10 and (masks["culled"] & on).sum() >= 10
    for k in R.ARRAYS:
        assert (got[k][zero].view(np.uint32) == 0).all(), k
        assert (got[k][:, 3].view(np.uint32) == 0).all() or k == "rotations"
        assert np.isfinite(got[k]).all()
    # the three vector gradients against (b), with the leave-out rule
    clean = {k: np.where(np.isfinite(v), v, 1.0).astype(np.float32) for k, v in scene.items()}       # (rows that are off anyway)
    near, _ = R.near_a_threshold(clean, cam, semantics)
    ref, _ = R.gradients(clean, cam, np.where(on, g, 0.0).astype(np.float32), semantics, masks=masks)
    keep = ~near
    for k in R.ARRAYS:
        width = ref[k].shape[1]
        top = float(np.abs(ref[k][keep]).max())
        err = float(np.abs(got[k][:, :width].astype(np.float64) - ref[k])[keep].max()) / top
        print(f"[antialias] {semantics} dL_d{k}: error {err:.2e} of the largest entry {top:.3e} (bound {R.bound((semantics, 'conditioned'), k):.1e})")
        assert top > 0 and err <= R.bound((semantics, "conditioned"), k), (k, err)
    assert all(_same_bits(before[k], t[k]) for k in t), "an input was written"


@pytest.mark.parametrize("semantics", PROFILES)
def test_backward_outputs_alone_twice_and_without_radii(semantics):
    cam = R.camera(semantics)
    scene, g, radii, _ = _backward_case(semantics, 257)
    n = len(g)
    t, gd, rd = _inputs(scene, cam), _dev(g), _dev(radii, np.int32)
    both = _backward(t, n, cam, semantics, gd, rd)
    again = _backward(t, n, cam, semantics, gd, rd)
    assert all(_same_bits(both[k], again[k]) for k in both)
    for k in BACKWARD_OUTPUTS:
        alone = _backward(t, n, cam, semantics, gd, rd, outputs=(k,))
        assert _same_bits(alone[k], both[k]), k
    # radii == NULL: every row with g != 0 is computed; the rows that had a tile are the same bits
    free = _backward(t, n, cam, semantics, gd, None)
    had = radii > 0
    for k in both:
        assert (_bits(free[k])[had] == _bits(both[k])[had]).all(), k
    assert (free["opacities"].cpu().numpy()[~had & (g != 0)] != 0).any()


@pytest.mark.parametrize("semantics", PROFILES)
def test_backward_on_needles_is_finite(semantics):
    cam, scene = R.camera(semantics), R.needle_scene(semantics)
    n = scene["opacities"].shape[0]
    for mod in (1.0, 0.5, 2.0):
        got = _backward(_inputs(scene, cam), n, cam, semantics, _dev(R.seed_gradient(n, seed=6)), None, scale_modifier=mod)
        masks = R.masks_of(scene, cam, semantics, mod)
        for k, v in got.items():
            v = v.cpu().numpy()
            assert np.isfinite(v).all(), (k, mod)
            if k != "opacities":
                assert (v[~masks["flows"]].view(np.uint32) == 0).all() and (v[masks["flows"]] != 0).any(), (k, mod)


# ---- composition with the rasterizer ----------------------------------------------------------------------------------------------
DRAW = dict(plan="sort", tile_history=False)
RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
BG = (0.1, 0.2, 0.3)


def _params(semantics):
    from gsrast_amd.autograd import GaussianParams
    raw = R.composition_raw(semantics)
    return GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if semantics == "inria" else "file", device="cuda:0")


def _rasterizer():
    from gsrast_amd.rasterizer import SplatRasterizer
    return SplatRasterizer(R.CW, R.CH, background=BG)


@functools.lru_cache(maxsize=None)
def _weights():
    rng = np.random.default_rng(17)
    return _dev(rng.normal(size=(3, R.CH, R.CW))), _dev(1.0 + 0.25 * rng.normal(size=(R.CH, R.CW)))


def _loss(color, dmap):
    w, wd = _weights()
    return (w * color).sum() + (wd * dmap).sum()


@pytest.mark.parametrize("semantics", PROFILES)
def test_antialiased_frame_is_the_frame_of_the_compensated_opacities(semantics):
    torch = _torch()
    from gsrast_amd import autograd
    cam, kw = R.composition_camera(), dict(semantics=semantics, sh_degree=3, depth=True, **DRAW)
    params, rast, slot = _params(semantics), _rasterizer(), autograd.RadiiSlot()
    color, dmap, omap = autograd.render(params, rast, cam, antialiased=True, radii_slot=slot, **kw)
    conic_w = rast.map_geometry_state()["conicOpacity"][:, 3].clone()
    _loss(color, dmap).backward()
    # the same frame by hand: the device's activations, c from the float32 restatement, o c as a leaf
    with torch.no_grad():
        act = autograd.activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
    scene = {k: v.cpu().numpy() for k, v in zip(("means3D", "scales", "rotations", "opacities"), act)}
    masks = R.masks_of(scene, cam, semantics)
    flows = masks["flows"]
    assert 0.35 <= float((masks["c"][flows] < 0.9).mean()) <= 0.75
    leaves = [a.clone().requires_grad_(True) for a in act[:3]] + [_dev(masks["o_out"]).requires_grad_(True)]
    shs = params.shs.detach().clone().requires_grad_(True)
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, rast.device)
    rast2, slot2 = _rasterizer(), autograd.RadiiSlot()
    color2, dmap2, omap2 = autograd.rasterize(rast2, *leaves, shs, view, proj, cam_pos, (tx, ty), radii_slot=slot2, **kw)
    assert _same_bits(color, color2) and _same_bits(dmap, dmap2) and _same_bits(omap, omap2)
    radii = slot.radii.cpu().numpy()
    assert np.array_equal(radii, slot2.radii.cpu().numpy()) and (radii > 0).sum() > 100 and (radii <= 0).sum() >= 10
    vis = radii > 0
    assert np.array_equal(_bits(conic_w)[vis], masks["o_out"].view(np.int32)[vis])
    _loss(color2, dmap2).backward()
    # expected raw gradients: the leaf run's, plus (b)'s seeded with that run's dL/do', through the activation reference
    g = leaves[3].grad.cpu().numpy()
    assert (g[~vis] == 0).all() and (g[vis] != 0).sum() > 50
    ref, _ = R.gradients(scene, cam, g, semantics, masks=masks)
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 4 - a.shape[1]))], 1)
    total = [leaves[i].grad.cpu().numpy().astype(np.float64) + pad(ref[k]) for i, k in enumerate(R.ARRAYS)]
    raw = R.composition_raw(semantics)
    want = dict(zip(("xyz", "opacity_logit", "log_scale", "rotation"),
                    A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], *total, ref["opacities"], radii=radii)))
    near, _ = R.near_a_threshold(scene, cam, semantics)
    keep = ~near
    bound = max(R.bound((semantics, "composition"), k) for k in R.ARRAYS)
    for k, w in want.items():
        got = getattr(params, k).grad.cpu().numpy().astype(np.float64)
        top = float(np.abs(w[keep]).max())
        err = float(np.abs(got - w)[keep].max()) / top
        # the compensation's own share of the gradient, so that a backward that dropped it would show
        plain = dict(zip(("xyz", "opacity_logit", "log_scale", "rotation"),
                         A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"],
                                    *[leaves[i].grad.cpu().numpy().astype(np.float64) for i in range(3)], g.astype(np.float64), radii=radii)))[k]
        share = float(np.abs(plain - w)[keep].max()) / top
        print(f"[antialias] {semantics} {k}.grad: error {err:.2e} of the largest entry {top:.3e}; without the compensation's gradient {share:.2e}")
        assert top > 0 and err <= bound, (k, err)
        assert share > 2 * bound, (k, share)
        assert (got[~vis] == 0).all(), k
    assert _same_bits(params.shs.grad, shs.grad)


@pytest.mark.parametrize("semantics", PROFILES)
def test_default_path_is_untouched_and_a_differentiable_view_is_refused(semantics):
    torch = _torch()
    from gsrast_amd import autograd
    cam, kw = R.composition_camera(), dict(semantics=semantics, sh_degree=3, depth=True, **DRAW)
    runs = []
    for extra in ({}, {"antialiased": False}):
        params = _params(semantics)
        color, dmap, omap = autograd.render(params, _rasterizer(), cam, **kw, **extra)
        _loss(color, dmap).backward()
        runs.append([color, dmap, omap] + [getattr(params, k).grad for k in RAW])
    assert all(_same_bits(a, b) for a, b in zip(*runs))
    # ... and the antialiased frame is another one: darker where small splats were spread at full opacity
    color_aa, _, omap_aa = autograd.render(_params(semantics), _rasterizer(), cam, antialiased=True, **kw)
    assert not _same_bits(color_aa, runs[0][0]) and float(omap_aa.sum()) < float(runs[0][2].sum())
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, torch.device("cuda:0"))
    with pytest.raises(ValueError, match="view"):
        autograd.render(_params(semantics), _rasterizer(), (view.clone().requires_grad_(True), proj, cam_pos, tx, ty), antialiased=True, **kw)
    # (a projection or camera position that requires a gradient is fine: c does not vary with them)
    moving = (view, proj.clone().requires_grad_(True), cam_pos.clone().requires_grad_(True), tx, ty)
    color, dmap, _ = autograd.render(_params(semantics), _rasterizer(), moving, antialiased=True, **kw)
    _loss(color, dmap).backward()
    assert moving[1].grad is not None and bool(torch.isfinite(moving[1].grad).all())


def test_five_antialiased_training_steps():
    torch = _torch()
    from gsrast_amd import autograd
    from gsrast_amd.optim import GaussianAdam
    semantics = "inria"
    cam, rast, kw = R.composition_camera(), _rasterizer(), dict(semantics=semantics, sh_degree=3, antialiased=True)
    with torch.no_grad():
        target = autograd.render(_params(semantics), rast, cam, **kw)[0]
    params = _params(semantics)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, amp in (("xyz", 0.02), ("opacity_logit", 0.5), ("log_scale", 0.2), ("rotation", 0.1), ("shs", 0.1)):
            p = getattr(params, k)
            p.add_((amp * torch.randn(p.shape, generator=gen)).to(p.device))
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    slot, losses = autograd.RadiiSlot(), []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        loss = (autograd.render(params, rast, cam, radii_slot=slot, **kw)[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        if len(losses) <= 5:
            loss.backward()
            culled = slot.radii <= 0
            assert int(culled.sum()) >= 10
            for k in RAW:
                grad = getattr(params, k).grad
                assert bool(torch.isfinite(grad).all()) and bool((grad[culled] == 0).all()), k
            opt.step(slot.radii)
    print(f"[antialias] L1 loss over five steps: {' '.join(f'{v:.6f}' for v in losses)}")
    assert all(np.isfinite(losses)) and losses[0] > 0
    assert losses[-1] < losses[0]
