"""GPU: adaptive density control — gsr_densify_accumulate, gsr_densify_plan + gsr_densify_apply and gsrast_amd.densify —
bit for bit against the numpy reference (tests/densify_ref.py; tests/test_densify_cpu.py shows that the seeded scenes meet
every class), with sentinels around everything a kernel writes; autograd.FrameSlot against a hand-run backward; and a
short training run that densifies half way."""
import ctypes as C

import numpy as np
import pytest

import densify_ref as R
from test_densify_cpu import PLAN_SIZES, reference_of

pytestmark = pytest.mark.gpu

SENTINEL = -7
GAP = 64                                 # sentinel elements on both sides of every array
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Arena:
    """One device buffer of 4-byte elements filled with a sentinel; every array is a 16-byte-aligned slice of it, GAP
    sentinels on both sides. `host` is what the buffer is expected to hold."""

    def __init__(self, dtype, sizes):
        import torch
        self.slices, at = {}, GAP
        for name, count in sizes.items():
            self.slices[name] = slice(at, at + count)
            at += (count + 3) // 4 * 4 + GAP
        self.host = np.full(at, SENTINEL, dtype)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def put(self, name, a):
        import torch
        a = np.ascontiguousarray(a, self.host.dtype).reshape(-1)
        assert a.size == self.slices[name].stop - self.slices[name].start, name
        self.host[self.slices[name]] = a
        self.dev[self.slices[name]] = torch.from_numpy(a).cuda()

    def expect(self, name, a, at=0):
        a = np.ascontiguousarray(a, self.host.dtype).reshape(-1)
        start = self.slices[name].start + at
        assert start + a.size <= self.slices[name].stop, name
        self.host[start:start + a.size] = a

    def tensor(self, name, *shape):
        t = self.dev[self.slices[name]]
        t = t.view(*shape) if shape else t
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        return t

    def ptr(self, name):
        return self.dev.data_ptr() + 4 * self.slices[name].start

    def mismatches(self):
        """Where the device buffer differs from `host`, bit for bit: the names of the arrays, or 'sentinel'."""
        import torch
        torch.cuda.synchronize()
        diff = _bits(self.dev.cpu().numpy()) != _bits(self.host)
        where = []
        for name, q in self.slices.items():
            if diff[q].any():
                where.append(f"{name} at {np.nonzero(diff[q])[0][:8].tolist()}")
                diff[q] = False
        if diff.any():
            where.append(f"sentinel at {np.nonzero(diff)[0][:8].tolist()}")
        return where


# ---- 1. accumulate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["all", "none", "alternating", "wave_culled", "last_row", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4097])
def test_accumulate_is_the_reference_bit_for_bit(n, kind):
    """Two frames in a row through DensityStats.update on top of statistics that are not zero, NaN gradients in the rows a
    frame culled; after each the WHOLE buffers are compared: visible rows updated, culled rows, inputs and sentinels as
    they were."""
    from gsrast_amd.autograd import FrameSlot
    from gsrast_amd.densify import DensityStats
    from test_gpu_adam import _visibility
    rng = np.random.default_rng(1000 * n + len(kind))
    fl = _Arena(F, {"grad": 2 * n, "grad_accum": n})
    it = _Arena(np.int32, {"radii": n, "denom": n, "max_radii": n})
    fl.put("grad_accum", 10.0 ** rng.uniform(-5, -2, n))
    it.put("denom", rng.integers(0, 50, n))
    it.put("max_radii", rng.integers(0, 100, n))
    stats = DensityStats(0, "cuda:0")
    stats.grad_accum, stats.denom, stats.max_radii = fl.tensor("grad_accum"), it.tensor("denom"), it.tensor("max_radii")
    slot = FrameSlot()
    slot.radii, slot.dL_dmean2D = it.tensor("radii"), fl.tensor("grad", n, 2)
    width, height = 1920, 1080
    for frame in range(2):
        radii = _visibility(kind, n, rng)
        grad = (rng.normal(size=(n, 2)) * 10.0 ** rng.uniform(-7, -3, (n, 1))).astype(F)
        grad[radii <= 0] = np.nan
        fl.put("grad", grad)
        it.put("radii", radii)
        before = fl.host.copy()
        stats.update(slot, width, height)
        sl = lambda arena, name: arena.host[arena.slices[name]]
        acc, den, big = R.accumulate(grad, radii, 0.5 * width, 0.5 * height, sl(fl, "grad_accum"), sl(it, "denom"), sl(it, "max_radii"))
        fl.expect("grad_accum", acc)
        it.expect("denom", den)
        it.expect("max_radii", big)
        assert fl.mismatches() == [] and it.mismatches() == [], (frame, kind)
        assert (_bits(before) != _bits(fl.host)).any() == bool((radii > 0).any())     # (the reference itself moved something)


# ---- 2. plan + apply --------------------------------------------------------------------------------------------------------
def _activations(raw):
    """The standard deviations and the normalised quaternions as the device forms them (gsr_activate_params)."""
    import torch
    from gsrast_amd.autograd import activate
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    with torch.no_grad():
        _, scales, rotations, _ = activate(up(raw["xyz"]), up(raw["opacity_logit"]), up(raw["log_scale"]), up(raw["rotation"]))
    return scales.cpu().numpy()[:, :3].copy(), rotations.cpu().numpy().copy()


def _reference(case, moments):
    stds, quats = _activations(case["raw"])
    return R.densify(case["raw"], case["moments"] if moments else {}, case["grad_accum"], case["denom"], case["max_radii"],
                     case["scalars"], case["max_screen"], case["noise"], stds, quats)


def _plan_and_apply(case, moments, want):
    """The two C calls on arenas: the plan's outputs against `want`, then the apply with destination arrays of the sizes
    the plan gave. Every buffer a kernel writes is compared whole."""
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    raw = case["raw"]
    n = raw["xyz"].shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src = {k: up(raw[k]) for k in R.RAW}
    src_m = {k: tuple(up(a) for a in case["moments"][k]) for k in R.RAW} if moments else {}
    stat = [up(case["grad_accum"]), up(case["denom"]), up(case["max_radii"])]
    it = _Arena(np.int32, {"src_of": 3 * n, "counts": 4})
    temp = torch.full((int(L.gsr_densify_plan_temp_bytes(n)) + 2 * GAP,), 0x5A, dtype=torch.uint8).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    scalars = [float(s) for s in case["scalars"]]
    rc = L.gsr_densify_plan(n, src["opacity_logit"].data_ptr(), src["log_scale"].data_ptr(), *(t.data_ptr() for t in stat), *scalars,
                            int(case["max_screen"]), temp.data_ptr() + GAP, it.ptr("src_of"), it.ptr("counts"), stream)
    assert rc == _capi.GSR_OK
    total = want["counts"][3]
    it.expect("counts", want["counts"])
    it.expect("src_of", want["src_of"])                       # (rows [N_new, 3 n) of src_of stay the sentinel)
    assert it.mismatches() == []
    guard = temp.cpu().numpy()
    assert (guard[:GAP] == 0x5A).all() and (guard[-GAP:] == 0x5A).all()      # the scratch's two ends
    # ---- apply ----
    names = [(k, part) for k in R.RAW for part in (("p", "m", "v") if moments else ("p",))]
    fl = _Arena(F, {f"{k}.{part}": total * R.WIDTHS[k] for k, part in names})
    splits = want["counts"][2]
    noise = up(case["noise"][:max(splits, 1)])
    a = _capi.DensifyApplyArgs()
    a.struct_size, a.log_shrink, a.n_src = C.sizeof(_capi.DensifyApplyArgs), scalars[4], n
    a.counts[:] = list(want["counts"])
    a.src_of, a.noise, a.stream = it.ptr("src_of"), noise.data_ptr(), stream
    for k in R.RAW:
        arr = getattr(a, k)
        arr.src, arr.dst = src[k].data_ptr(), fl.ptr(f"{k}.p")
        if moments:
            arr.src_exp_avg, arr.src_exp_avg_sq = src_m[k][0].data_ptr(), src_m[k][1].data_ptr()
            arr.dst_exp_avg, arr.dst_exp_avg_sq = fl.ptr(f"{k}.m"), fl.ptr(f"{k}.v")
    assert L.gsr_densify_apply(C.byref(a)) == _capi.GSR_OK
    for k in R.RAW:
        fl.expect(f"{k}.p", want["raw"][k])
        if moments:
            fl.expect(f"{k}.m", want["moments"][k][0])
            fl.expect(f"{k}.v", want["moments"][k][1])
    assert fl.mismatches() == [] and it.mismatches() == []
    # the sources are as they were
    torch.cuda.synchronize()
    for k in R.RAW:
        assert (_bits(src[k].cpu().numpy()) == _bits(raw[k])).all(), k


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
@pytest.mark.parametrize("n", PLAN_SIZES)
def test_plan_and_apply_are_the_reference_bit_for_bit(n, moments):
    case, _ = reference_of(n)
    want = _reference(case, moments)
    print(f"[densify] n={n}: counts {want['counts']}")
    _plan_and_apply(case, moments, want)


def _degenerate(kind, n):
    """The seeded scene of n rows under thresholds that leave one class only."""
    case, _ = reference_of(n)
    case = dict(case)
    max_grad, log_dense, logit_min, log_world, log_shrink = case["scalars"]
    never, always = F(1e30), F(1e-30)
    case["denom"], case["grad_accum"] = np.ones(n, np.int32), np.ones(n, F)           # every Gaussian was seen and has a gradient
    if kind == "identity":
        case["scalars"], case["max_screen"] = (never, log_dense, -never, log_world, log_shrink), 0
    elif kind == "all_pruned":
        case["scalars"] = (max_grad, log_dense, never, log_world, log_shrink)
    elif kind == "all_clone":
        case["scalars"], case["max_screen"] = (always, never, -never, log_world, log_shrink), 0
    elif kind == "all_split":
        case["scalars"], case["max_screen"] = (always, -never, -never, log_world, log_shrink), 0
    else:
        assert kind == "children_doomed"                                                 # parents and children alike too large for the world
        case["scalars"], case["max_screen"] = (always, -never, -never, -never, log_shrink), 1000
    return case


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
@pytest.mark.parametrize("kind", ["identity", "all_pruned", "all_clone", "all_split", "children_doomed"])
def test_degenerate_plans(kind, moments):
    n = 321
    case = _degenerate(kind, n)
    want = _reference(case, moments)
    expect = {"identity": (n, 0, 0, n), "all_pruned": (0, 0, 0, 0), "all_clone": (n, n, 0, 2 * n), "all_split": (0, 0, n, 2 * n),
              "children_doomed": (0, 0, 0, 0)}[kind]
    assert want["counts"] == expect
    if kind == "identity":
        assert np.array_equal(want["src_of"], np.arange(n))
        for k in R.RAW:
            assert (_bits(want["raw"][k]) == _bits(case["raw"][k])).all()
            if moments:
                assert all((_bits(a) == _bits(b)).all() for a, b in zip(want["moments"][k], case["moments"][k]))
    _plan_and_apply(case, moments, want)


# ---- 3. the Python layer ----------------------------------------------------------------------------------------------------
WITHOUT_STATE = "rotation"               # the optimiser has never stepped this parameter: it gets no moments
SEED = 11


def _trainer(case):
    """GaussianParams, a GaussianAdam with a group per array (state as after seven steps, but none for WITHOUT_STATE) and the
    statistics of the seeded case, on the device."""
    import torch
    from gsrast_amd.autograd import GaussianParams
    from gsrast_amd.densify import DensityStats
    from gsrast_amd.optim import GaussianAdam
    raw = case["raw"]
    n = raw["xyz"].shape[0]
    params = GaussianParams.from_raw(*(raw[k] for k in R.RAW), device="cuda:0")
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": 1e-3 * (i + 1)} for i, k in enumerate(R.RAW)])
    for k in R.RAW:
        if k != WITHOUT_STATE:
            m, v = (torch.from_numpy(a.copy()).cuda() for a in case["moments"][k])
            opt.state[getattr(params, k)].update(step=7, exp_avg=m, exp_avg_sq=v)
    stats = DensityStats(n, "cuda:0")
    stats.grad_accum.copy_(torch.from_numpy(case["grad_accum"]))
    stats.denom.copy_(torch.from_numpy(case["denom"]))
    stats.max_radii.copy_(torch.from_numpy(case["max_radii"]))
    return params, opt, stats


def _densify(case, params, opt, stats):
    import torch
    from gsrast_amd.densify import densify_and_prune
    return densify_and_prune(params, opt, stats, max_grad=2e-4, min_opacity=0.005, extent=case["extent"], max_screen_size=case["max_screen"],
                             percent_dense=0.01, generator=torch.Generator().manual_seed(SEED))


def test_densify_and_prune_swaps_parameters_and_state_in_place():
    import torch
    n = 1366
    case, first = reference_of(n)
    splits = first["counts"][2]                                                          # (the counts do not depend on the noise)
    case = dict(case, noise=torch.randn((splits, 2, 3), generator=torch.Generator().manual_seed(SEED)).numpy())
    stds, quats = _activations(case["raw"])
    moments = {k: v for k, v in case["moments"].items() if k != WITHOUT_STATE}
    want = R.densify(case["raw"], moments, case["grad_accum"], case["denom"], case["max_radii"], case["scalars"], case["max_screen"],
                     case["noise"], stds, quats)
    assert want["counts"] == first["counts"] and splits > 0
    params, opt, stats = _trainer(case)
    old = {k: getattr(params, k) for k in R.RAW}
    lists = [g["params"] for g in opt.param_groups]
    src_of, counts = _densify(case, params, opt, stats)
    torch.cuda.synchronize()
    total = want["counts"][3]
    assert tuple(counts) == want["counts"] and src_of.dtype == torch.int32 and np.array_equal(src_of.cpu().numpy(), want["src_of"])
    host = lambda t: t.detach().cpu().numpy()
    for i, k in enumerate(R.RAW):
        p = getattr(params, k)
        assert isinstance(p, torch.nn.Parameter) and p is not old[k] and p.requires_grad and p.grad is None
        assert (_bits(host(p)) == _bits(want["raw"][k])).all() and host(p).shape == want["raw"][k].shape, k
        assert opt.param_groups[i]["params"] is lists[i]                                 # the list object, swapped in place
        assert lists[i][0] is p and len(lists[i]) == 1 and opt.param_groups[i]["lr"] == 1e-3 * (i + 1)
        assert old[k] not in opt.state
        if k == WITHOUT_STATE:
            assert p not in opt.state                                                    # no state before, none made
        else:
            st = opt.state[p]
            assert st["step"] == 7 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
            for name, w in zip(("exp_avg", "exp_avg_sq"), want["moments"][k]):
                assert (_bits(host(st[name])) == _bits(w)).all() and st[name].shape == p.shape, (k, name)
    assert len(opt.state) == len(R.RAW) - 1
    for t, dtype in ((stats.grad_accum, torch.float32), (stats.denom, torch.int32), (stats.max_radii, torch.int32)):
        assert tuple(t.shape) == (total,) and t.dtype == dtype and not t.any()
    # the optimiser goes on: a step over the new rows
    for k in R.RAW:
        getattr(params, k).grad = torch.ones_like(getattr(params, k))
    opt.step()
    assert opt.state[params.xyz]["step"] == 8 and opt.state[params.rotation]["step"] == 1
    # the same seed again gives the same bits; without an optimiser the parameters are the same
    again, again_opt, again_stats = _trainer(case)
    _densify(case, again, again_opt, again_stats)
    bare, _, bare_stats = _trainer(case)
    _, bare_counts = _densify(case, bare, None, bare_stats)
    assert tuple(bare_counts) == want["counts"]
    for k in R.RAW:
        assert (_bits(host(getattr(again, k))) == _bits(want["raw"][k])).all(), k
        assert (_bits(host(getattr(bare, k))) == _bits(want["raw"][k])).all(), k


def test_every_refusal_leaves_parameters_and_optimiser_untouched():
    import torch
    from gsrast_amd.densify import DensityStats
    from gsrast_amd.optim import GaussianAdam
    case, _ = reference_of(65)

    def snapshot(params, opt):
        return ([id(getattr(params, k)) for k in R.RAW], [[id(p) for p in g["params"]] for g in opt.param_groups],
                {id(p): {k: (id(v) if isinstance(v, torch.Tensor) else v) for k, v in st.items()} for p, st in opt.state.items()})

    def refused(message, change):
        params, opt, stats = _trainer(case)
        params, opt, stats = change(params, opt, stats) or (params, opt, stats)
        before, values = snapshot(params, opt), [getattr(params, k).detach().clone() for k in R.RAW]
        with pytest.raises(ValueError, match=message):
            _densify(case, params, opt, stats)
        assert snapshot(params, opt) == before
        assert all(torch.equal(v, getattr(params, k).detach()) for v, k in zip(values, R.RAW))

    def other_optimiser(params, opt, stats):
        return params, GaussianAdam([params.xyz, params.opacity_logit, params.log_scale, params.rotation]), stats

    def moment_of(dtype=None, rows=None, alone=False):
        def change(params, opt, stats):
            st = opt.state[params.log_scale]
            if alone:
                del st["exp_avg_sq"]
            else:
                st["exp_avg"] = torch.zeros((rows or 65, 3), dtype=dtype or torch.float32, device="cuda:0")
        return change

    def parameter(make):
        def change(params, opt, stats):
            old = params.rotation
            params.rotation = torch.nn.Parameter(make(old.detach()))
            opt.param_groups[3]["params"][0] = params.rotation
        return change

    refused("does not hold shs", other_optimiser)
    refused("statistics", lambda p, o, s: (p, o, DensityStats(64, "cuda:0")))
    refused("statistics", lambda p, o, s: (p, o, DensityStats(65, "cpu")))
    refused("state exp_avg of log_scale is torch.float64", moment_of(dtype=torch.float64))
    refused(r"state exp_avg of log_scale is \(64, 3\)", moment_of(rows=64))
    refused("exp_avg alone", moment_of(alone=True))
    refused("rotation is torch.float64", parameter(lambda t: t.double()))
    refused("rotation is on cpu", parameter(lambda t: t.cpu()))
    refused("rotation is not contiguous", parameter(lambda t: torch.zeros((65, 8), device="cuda:0")[:, :4]))
    refused(r"rotation is \(64, 4\)", parameter(lambda t: t[:64].clone()))


def test_reset_opacity_against_numpy():
    import torch
    from gsrast_amd.densify import reset_opacity
    case, _ = reference_of(1365)
    params, opt, _ = _trainer(case)
    p = params.opacity_logit
    st = opt.state[p]
    versions = [t._version for t in (p, st["exp_avg"], st["exp_avg_sq"])]
    reset_opacity(params, opt, ceiling=0.01)
    torch.cuda.synchronize()
    raw = case["raw"]["opacity_logit"]
    want = np.minimum(raw, F(np.log(0.01 / 0.99)))
    assert (want != raw).any() and (want == raw).any()
    assert (_bits(p.detach().cpu().numpy()) == _bits(want)).all()
    assert not st["exp_avg"].any() and not st["exp_avg_sq"].any() and st["step"] == 7
    assert all(t._version > v for t, v in zip((p, st["exp_avg"], st["exp_avg_sq"]), versions))
    others = [k for k in R.RAW if k not in ("opacity_logit", WITHOUT_STATE)]
    assert all(opt.state[getattr(params, k)]["exp_avg"].any() for k in others)       # (nothing else was zeroed)
    reset_opacity(params, None)                                                          # no optimiser: the clamp alone


# ---- 4. FrameSlot -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("profile", ["gscuda", "inria"])
def test_frame_slot_carries_the_backwards_dL_dmean2D(profile):
    import torch
    from gsrast_amd.autograd import FrameSlot, RadiiSlot, render
    from test_gpu_autograd import DRAW, RAW, _cam, _kw, _params, _rasterizer, _same_bits, _weights
    wt = _weights()[0]
    cam = _cam(1)
    grads = {}
    for name, slot in (("frame", FrameSlot()), ("radii", RadiiSlot())):
        params, rast = _params(profile), _rasterizer()
        (wt * render(params, rast, cam, radii_slot=slot, **_kw(profile), **DRAW)[0]).sum().backward()
        grads[name] = [getattr(params, k).grad for k in RAW]
        if name == "frame":
            n = params.num_gaussians
            got = slot.dL_dmean2D
            assert got.dtype == torch.float32 and tuple(got.shape) == (n, 2) and tuple(slot.radii.shape) == (n,)
            # the same frame's backward by hand, on the rasterizer that still holds it
            hand = rast.backward(wt, outputs=("dL_dmean2D", "dL_dconic_opacity"), wide_sums=True, **_kw(profile))["dL_dmean2D"]
            assert got.data_ptr() != hand.data_ptr() and _same_bits(got, hand)
            assert bool((got[slot.radii > 0] != 0).any()) and not bool(got[slot.radii <= 0].any())
        else:
            assert not hasattr(slot, "dL_dmean2D") and slot.radii is not None
    torch.cuda.synchronize()
    for a, b, k in zip(grads["frame"], grads["radii"], RAW):
        assert _same_bits(a, b), k


# ---- 5. a small training run ------------------------------------------------------------------------------------------------
def _train(densify, steps=(8, 8)):
    """tests/test_gpu_adam.py's sparse training run (168 Gaussians, eight of them behind the camera) with a FrameSlot and
    DensityStats; after steps[0] steps `densify(params, opt, stats)` is called (None: no call), then steps[1] more through
    the same SplatRasterizer. -> losses, final arrays, what densify returned"""
    import torch
    from gsrast_amd.autograd import FrameSlot, GaussianParams, render
    from gsrast_amd.densify import DensityStats
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_adam import EXTRA
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer
    profile = "inria"
    cam, rast = _cam(1), _rasterizer()
    raw = {k: v.copy() for k, v in _raw_scene(profile).items()}
    rng = np.random.default_rng(9)
    eye = np.asarray(cam.cam_pos, np.float64).reshape(-1)[:3]
    back = eye / np.linalg.norm(eye)
    tail = {k: raw[k][:EXTRA].copy() for k in RAW}
    tail["xyz"] = (eye + back * rng.uniform(1.0, 3.0, (EXTRA, 1)) + 0.3 * rng.normal(size=(EXTRA, 3))).astype(np.float32)
    raw = {k: np.concatenate([raw[k], tail[k]]) for k in RAW}
    make = lambda: GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major", device="cuda:0")
    with torch.no_grad():
        target = render(make(), rast, cam, **_kw(profile))[0]
    params = make()
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, amp in (("xyz", 0.02), ("opacity_logit", 0.5), ("log_scale", 0.2), ("rotation", 0.1), ("shs", 0.1)):
            p = getattr(params, k)
            p.add_((amp * torch.randn(p.shape, generator=gen)).to(p.device))
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    slot, stats = FrameSlot(), DensityStats(params.num_gaussians, "cuda:0")
    losses, returned = [], None
    for step in range(sum(steps)):
        if step == steps[0] and densify is not None:
            returned = densify(params, opt, stats)
        n = params.num_gaussians
        opt.zero_grad(set_to_none=True)
        loss = (render(params, rast, cam, radii_slot=slot, **_kw(profile))[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        loss.backward()
        assert rast.num_gaussians == n and tuple(slot.radii.shape) == (n,) and tuple(slot.dL_dmean2D.shape) == (n, 2)
        for k in RAW:
            assert getattr(params, k).grad.shape == getattr(params, k).shape and getattr(params, k).shape[0] == n, k
        opt.step(slot.radii)
        stats.update(slot, rast.width, rast.height)
    torch.cuda.synchronize()
    return losses, [getattr(params, k).detach().clone() for k in RAW], returned


def test_a_training_run_that_densifies_half_way():
    import torch
    from gsrast_amd.densify import densify_and_prune
    from test_gpu_autograd import RAW, _same_bits
    seen = {}

    def densify(params, opt, stats):
        """Thresholds from the statistics themselves — the median mean gradient of the Gaussians seen, the median size —
        so that about half of them are hot and about half of those big; the reference's plan for them must not be trivial."""
        host = lambda t: t.detach().cpu().numpy().copy()
        raw = {k: host(getattr(params, k)) for k in RAW}
        ga, den, big = host(stats.grad_accum), host(stats.denom), host(stats.max_radii)
        g = R.mean_gradient(ga, den)
        max_grad = float(np.median(g[den > 0]))
        extent = float(np.median(np.exp(raw["log_scale"].max(axis=1).astype(np.float64)))) / 0.01
        kw = dict(max_grad=max_grad, min_opacity=0.005, extent=extent, max_screen_size=None, percent_dense=0.01)
        stds, quats = _activations(raw)
        moments = {k: tuple(host(opt.state[getattr(params, k)][m]) for m in ("exp_avg", "exp_avg_sq")) for k in RAW}
        probe = R.densify(raw, moments, ga, den, big, R.plan_scalars(max_grad, 0.005, extent), 0, np.zeros((len(g), 2, 3), F), stds, quats)
        noise = torch.randn((probe["counts"][2], 2, 3), generator=torch.Generator().manual_seed(3)).numpy()
        want = R.densify(raw, moments, ga, den, big, R.plan_scalars(max_grad, 0.005, extent), 0, noise, stds, quats)
        src_of, counts = densify_and_prune(params, opt, stats, generator=torch.Generator().manual_seed(3), **kw)
        seen.update(want=want, counts=counts, n=len(g), den=den)
        assert tuple(counts) == want["counts"] and np.array_equal(src_of.cpu().numpy(), want["src_of"])
        for k in RAW:
            assert (_bits(host(getattr(params, k))) == _bits(want["raw"][k])).all(), k
            for m, w in zip(("exp_avg", "exp_avg_sq"), want["moments"][k]):
                assert (_bits(host(opt.state[getattr(params, k)][m])) == _bits(w)).all(), (k, m)
        return counts

    losses, end, counts = _train(densify)
    kept, clones, splits, total = counts
    print(f"[densify training] {seen['n']} Gaussians -> {total}: {kept} kept, {clones} clones, {splits} split; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert seen["n"] == 168 and (seen["den"] == 0).any() and (seen["den"] > 0).any()
    assert clones > 0 and splits > 0 and 0 < kept < 168 and total != 168                # not a trivial plan
    assert all(np.isfinite(losses)) and all(a.shape[0] == total for a in end) and all(bool(torch.isfinite(a).all()) for a in end)
    # thresholds under which the plan is the identity: the run is the run without the call, bit for bit
    identity = lambda params, opt, stats: densify_and_prune(params, opt, stats, max_grad=1e30, min_opacity=1e-30, extent=1.0)[1]
    with_call, end_call, counts_call = _train(identity)
    without, end_without, _ = _train(None)
    assert tuple(counts_call) == (168, 0, 0, 168)
    assert with_call == without and all(_same_bits(a, b) for a, b in zip(end_call, end_without))
