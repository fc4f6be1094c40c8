"""GPU: 3DGS-MCMC — gsr_mcmc_noise, gsr_mcmc_plan, gsr_mcmc_relocate and gsrast_amd.mcmc — against the numpy reference
(tests/mcmc_ref.py; tests/test_mcmc_cpu.py pins that reference to the paper's conditions), with sentinels around everything a
kernel writes and the read-only inputs compared afterwards. Moves and integers are compared bit for bit; so is the noise. The
two values the relocation computes in double are held to one float32 ulp of the float64 reference."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import mcmc_ref as R
from test_gpu_densify import GAP, _Arena, _bits

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)             # 4097: across the edge of the scan's tile of 4096 flags
MIN_OPACITY = 0.005
THRESHOLD = F(math.log(MIN_OPACITY / (1.0 - MIN_OPACITY)))
ULP = 2.0 ** -23


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _activated(opacity_logit, log_scale=None, rotation=None):
    """(stds [n,3], quats [n,4], opacities [n]) as the device forms them (gsr_activate_params: the kernels' own functions)."""
    import torch
    from gsrast_amd.autograd import activate
    n = opacity_logit.shape[0]
    log_scale = np.zeros((n, 3), F) if log_scale is None else log_scale
    rotation = np.tile(np.array([1, 0, 0, 0], F), (n, 1)) if rotation is None else rotation
    with torch.no_grad():
        _, scales, rotations, opacities = activate(_up(np.zeros((n, 3), F)), _up(opacity_logit), _up(log_scale), _up(rotation))
    return scales.cpu().numpy()[:, :3].copy(), rotations.cpu().numpy().copy(), opacities.cpu().numpy().copy()


def _logit(o):
    return np.log(np.asarray(o, np.float64) / (1.0 - np.asarray(o, np.float64))).astype(F)


# ---- 1. noise ---------------------------------------------------------------------------------------------------------------
def _noise_scene(n, seed):
    """Opacities on both sides of the gate first (0.001, 0.005, 0.5, 0.999, cycled), quaternions that are not unit, scales
    six orders of magnitude apart."""
    rng = np.random.default_rng(seed)
    logit = _logit(np.resize(np.array([0.001, 0.005, 0.5, 0.999, 0.004, 0.006]), n))
    logit[6:] += rng.normal(size=max(0, n - 6)).astype(F) * F(0.05)
    return dict(xyz=rng.normal(size=(n, 3)).astype(F), opacity_logit=logit,
                log_scale=rng.uniform(math.log(1e-3), math.log(1e3), (n, 3)).astype(F),
                rotation=(rng.normal(size=(n, 4)) * rng.uniform(0.2, 5.0, (n, 1))).astype(F), noise=rng.normal(size=(n, 3)).astype(F))


@pytest.mark.parametrize("scaler", [0.37, 0.0])
@pytest.mark.parametrize("n", SIZES)
def test_noise_is_the_reference_bit_for_bit(n, scaler):
    import torch
    from gsrast_amd import mcmc
    case = _noise_scene(n, 100 + n)
    fl = _Arena(F, {"xyz": 3 * n, "opacity_logit": n, "log_scale": 3 * n, "rotation": 4 * n, "noise": 3 * n})
    for k, a in case.items():
        fl.put(k, a)
    params = types.SimpleNamespace(xyz=fl.tensor("xyz", n, 3), opacity_logit=fl.tensor("opacity_logit"), log_scale=fl.tensor("log_scale", n, 3),
                                   rotation=fl.tensor("rotation", n, 4))
    s, q, o = _activated(case["opacity_logit"], case["log_scale"], case["rotation"])
    _, _, g = _activated(R.gate_argument(o))                                  # the gate: the same device function on t
    want = R.noise(case["xyz"], case["noise"], F(scaler), s, q, g)
    version = params.xyz._version
    mcmc.inject_noise(params, scaler, noise=fl.tensor("noise", n, 3))
    fl.expect("xyz", want)
    assert fl.mismatches() == []                                             # xyz as the reference, every input and sentinel as it was
    assert params.xyz._version > version
    moved = _bits(want) != _bits(case["xyz"])
    if scaler == 0.0:
        assert not moved.any()                                               # x + 0: the bits stay
    else:
        assert moved[0].all() and (n < 4 or not moved[3].any())              # o = 0.001 moves; o = 0.999: the gate is 0 in float32
    torch.cuda.synchronize()


def test_noise_draws_its_own_tensor_and_refuses_a_stale_graph():
    import torch
    from gsrast_amd import mcmc
    from gsrast_amd.autograd import GaussianParams
    case = _noise_scene(300, 7)
    case["opacity_logit"][:] = _logit(0.001)
    shs = np.zeros((300, 48), F)
    make = lambda: GaussianParams.from_raw(case["xyz"], case["opacity_logit"], case["log_scale"], case["rotation"], shs, device="cuda:0")
    a, b, c = make(), make(), make()
    mcmc.inject_noise(a, 0.01, generator=torch.Generator().manual_seed(4))
    mcmc.inject_noise(b, 0.01, generator=torch.Generator().manual_seed(4))
    drawn = torch.randn((300, 3), generator=torch.Generator().manual_seed(4))
    mcmc.inject_noise(c, 0.01, noise=drawn.cuda())
    assert torch.equal(a.xyz, b.xyz) and torch.equal(a.xyz, c.xyz) and not torch.equal(a.xyz.detach().cpu(), torch.from_numpy(case["xyz"]))
    assert isinstance(a.xyz, torch.nn.Parameter) and a.xyz.requires_grad
    loss = (a.xyz * a.xyz).sum()                                             # saves xyz for its backward
    mcmc.inject_noise(a, 0.01, generator=torch.Generator().manual_seed(5))
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        loss.backward()
    for bad, what in ((drawn, "noise is on cpu"), (drawn.cuda().double(), "float64"), (drawn.cuda()[:299], r"\(299, 3\)"),
                      (torch.zeros((300, 6), device="cuda:0")[:, :3], "not contiguous")):
        with pytest.raises(ValueError, match=what):
            mcmc.inject_noise(b, 0.01, noise=bad)


# ---- 2. plan ----------------------------------------------------------------------------------------------------------------
def _plan_logits(kind, n, rng):
    x = (2.0 * rng.normal(size=n) - 4.0).astype(F)                            # about a third at or below the threshold
    if kind == "none":
        x = np.abs(x) + F(1.0)
    elif kind == "all":
        x = -np.abs(x) - F(6.0)
    elif kind == "edges":
        x[::3] = THRESHOLD                                                   # equal: dead
        x[1::3] = np.nextafter(THRESHOLD, F(np.inf))                         # its upper neighbour: alive
        x[2::3] = np.nextafter(THRESHOLD, F(-np.inf))                        # its lower neighbour: dead
    return x.astype(F)


@pytest.mark.parametrize("kind", ["mixed", "none", "all", "edges"])
@pytest.mark.parametrize("n", SIZES)
def test_plan_is_the_reference_bit_for_bit(n, kind):
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    logit = _plan_logits(kind, n, np.random.default_rng(200 + n))
    _, _, o = _activated(logit)
    dead_idx, weights, counts = R.plan(logit, THRESHOLD, o)
    if kind in ("none", "all"):
        assert counts == ((0, n) if kind == "none" else (n, 0))
    if kind == "edges":
        assert dead_idx.tolist() == [i for i in range(n) if i % 3 != 1]
    it = _Arena(np.int32, {"dead_idx": n, "counts": 2})
    fl = _Arena(F, {"opacity_logit": n, "weights": n})
    fl.put("opacity_logit", logit)
    temp = torch.full((int(L.gsr_mcmc_plan_temp_bytes(n)) + 2 * GAP,), 0x5A, dtype=torch.uint8).cuda()
    rc = L.gsr_mcmc_plan(n, fl.ptr("opacity_logit"), float(THRESHOLD), temp.data_ptr() + GAP, it.ptr("dead_idx"), fl.ptr("weights"),
                         it.ptr("counts"), torch.cuda.current_stream().cuda_stream)
    assert rc == _capi.GSR_OK
    it.expect("dead_idx", dead_idx)                                          # (rows [dead, n) of dead_idx stay the sentinel)
    it.expect("counts", counts)
    fl.expect("weights", weights)
    assert it.mismatches() == [] and fl.mismatches() == []
    guard = temp.cpu().numpy()
    assert (guard[:GAP] == 0x5A).all() and (guard[-GAP:] == 0x5A).all()
    assert not np.signbit(weights[weights == 0]).any()


def test_plan_of_no_rows_writes_zero_counts():
    import torch
    from gsrast_amd import _capi
    it = _Arena(np.int32, {"counts": 2})
    assert _capi.lib().gsr_mcmc_plan(0, None, 0.0, None, None, None, it.ptr("counts"), torch.cuda.current_stream().cuda_stream) == _capi.GSR_OK
    it.expect("counts", [0, 0])
    assert it.mismatches() == []


# ---- 3. relocate ------------------------------------------------------------------------------------------------------------
PARTS = ("p", "m", "v")


def _relocate_scene(n, seed):
    rng = np.random.default_rng(seed)
    raw = {k: rng.normal(size=(n, R.WIDTHS[k]) if k != "opacity_logit" else n).astype(F) for k in R.RAW}
    raw["opacity_logit"] = _logit(rng.uniform(0.01, 0.98, n))
    moments = {k: ((0.1 * rng.normal(size=raw[k].shape)).astype(F), (10.0 ** rng.uniform(-4, 0, raw[k].shape)).astype(F)) for k in R.RAW}
    return raw, moments


def _check_computed(got_logit, got_ls, raw, want, hit, what):
    """The two values step 2 computes, on the rows `hit`: within one float32 ulp of the float64 reference rounded to float32.
    Both sides round a double that agrees to far better than 2^-40, so they can only fall on either side of one rounding
    boundary. The shift shows through log_scale' = fl(log_scale + shift): a shift one ulp off moves the sum by at most
    2^-23 |shift|, and the sum's own rounding may then fall the other way once more: 2^-23 (|shift| + |log_scale'|).
    The rows that are not bit-equal are printed, not asserted."""
    w_logit = want["want64"]["opacity_logit"][hit].astype(F)
    assert np.isfinite(got_logit[hit]).all() and np.isfinite(got_ls[hit]).all(), what
    assert (np.abs(got_logit[hit].astype(np.float64) - w_logit) <= ULP * np.abs(w_logit)).all(), what
    shift = want["want64"]["shift"][hit].astype(F)
    w_ls = want["raw"]["log_scale"][hit]
    bound = ULP * (np.abs(shift.astype(np.float64))[:, None] + np.abs(w_ls.astype(np.float64)))
    assert (np.abs(got_ls[hit].astype(np.float64) - w_ls) <= bound).all(), what
    off = int((_bits(got_logit[hit]) != _bits(w_logit)).sum()), int((_bits(got_ls[hit]) != _bits(w_ls)).any(axis=1).sum())
    print(f"[mcmc relocate] {what}: {int(hit.sum())} rows updated; not bit-equal: {off[0]} opacity_logit, {off[1]} log_scale rows")


def _adopt_computed(want, got_logit, got_ls, hit, sampled, dst, n):
    """The expectation with the device's own rounding of the two computed values on the updated rows — and in their copies,
    which must be bitwise copies of what the device itself wrote."""
    logit, ls = want["raw"]["opacity_logit"].copy(), want["raw"]["log_scale"].copy()
    logit[hit], ls[hit] = got_logit[hit], got_ls[hit]
    if dst is not None:
        s, d = np.asarray(sampled, np.int64), np.asarray(dst, np.int64)
        ok = (s >= 0) & (s < n) & (d >= 0) & (d < n)
        logit[d[ok]], ls[d[ok]] = logit[s[ok]], ls[s[ok]]
    return logit, ls


def _relocate(raw, moments, sampled, dst, what, min_opacity=MIN_OPACITY):
    """One gsr_mcmc_relocate on an arena against the reference: the two computed values by _check_computed, everything else
    — every other value of every row of all fifteen arrays, and every sentinel — bit for bit. -> the reference's result"""
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    n, m = raw["xyz"].shape[0], len(sampled)
    parts = PARTS if moments else PARTS[:1]
    fl = _Arena(F, {f"{k}.{part}": n * R.WIDTHS[k] for k in R.RAW for part in parts})
    for k in R.RAW:
        fl.put(f"{k}.p", raw[k])
        if moments:
            fl.put(f"{k}.m", moments[k][0])
            fl.put(f"{k}.v", moments[k][1])
    idx = _Arena(np.int32, {"sampled": max(m, 1), "dst": max(m, 1)})
    idx.put("sampled", sampled if m else [0])
    idx.put("dst", dst if (m and dst is not None) else [0] * max(m, 1))
    temp_bytes = int(L.gsr_mcmc_relocate_temp_bytes(n))
    temp = torch.full((temp_bytes + 2 * GAP,), 0x5A, dtype=torch.uint8).cuda()
    a = _capi.McmcRelocateArgs()
    a.struct_size, a.min_opacity, a.n, a.m = C.sizeof(_capi.McmcRelocateArgs), min_opacity, n, m
    a.sampled, a.dst = idx.ptr("sampled"), idx.ptr("dst") if dst is not None else None
    a.temp, a.stream = temp.data_ptr() + GAP, torch.cuda.current_stream().cuda_stream
    for k in R.RAW:
        arr = getattr(a, k)
        arr.param = fl.ptr(f"{k}.p")
        if moments:
            arr.exp_avg, arr.exp_avg_sq = fl.ptr(f"{k}.m"), fl.ptr(f"{k}.v")
    _, _, o = _activated(raw["opacity_logit"])
    want = R.relocate(raw, moments or {}, sampled, dst, F(min_opacity), o)
    assert L.gsr_mcmc_relocate(C.byref(a)) == _capi.GSR_OK
    torch.cuda.synchronize()
    guard = temp.cpu().numpy()
    assert (guard[:GAP] == 0x5A).all() and (guard[-GAP:] == 0x5A).all()
    if m == 0:
        assert (guard == 0x5A).all()                                         # nothing touched, temp included
    else:
        words = guard[GAP:GAP + temp_bytes].view(np.int32)
        assert words[0] == want["rejected"] and (words[4:4 + n] == want["counts"]).all()
    got = fl.dev.cpu().numpy()
    got_logit, got_ls = got[fl.slices["opacity_logit.p"]], got[fl.slices["log_scale.p"]].reshape(n, 3)
    hit = want["counts"] > 0
    _check_computed(got_logit, got_ls, raw, want, hit, what)
    logit, ls = _adopt_computed(want, got_logit, got_ls, hit, sampled, dst, n)
    for k in R.RAW:
        fl.expect(f"{k}.p", {"opacity_logit": logit, "log_scale": ls}.get(k, want["raw"][k]))
        if moments:
            fl.expect(f"{k}.m", want["moments"][k][0])
            fl.expect(f"{k}.v", want["moments"][k][1])
    assert fl.mismatches() == [] and idx.mismatches() == [], what
    return want


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
@pytest.mark.parametrize("n", SIZES)
def test_relocate_random_draws(n, moments):
    """A third of the rows are destinations, the draws fall on the others, with repeats."""
    raw, mom = _relocate_scene(n, 300 + n)
    rng = np.random.default_rng(n)
    if n == 1:
        sampled, dst = [0], None                                             # (no other row to copy to)
    else:
        rows = rng.permutation(n)
        dst = np.sort(rows[:max(1, n // 3)])
        sampled = rng.choice(rows[max(1, n // 3):], size=dst.size)
    want = _relocate(raw, mom if moments else None, sampled, dst, f"n={n}")
    assert want["rejected"] == 0 and (n < 63 or want["counts"].max() >= 2)


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
def test_relocate_clamps_the_ratio_at_51(moments):
    """Every one of 60 samples is row 7: the row is updated once, as if drawn 50 times, and copied to 60 rows."""
    raw, mom = _relocate_scene(65, 1)
    dst = [i for i in range(65) if i != 7][:60]
    want = _relocate(raw, mom if moments else None, [7] * 60, dst, "one row 60 times")
    assert want["counts"][7] == 60
    _, _, o = _activated(raw["opacity_logit"])
    assert want["want64"]["shift"][7] == R.relocated(o[7], 51, F(MIN_OPACITY))[3] != R.relocated(o[7], 61, F(MIN_OPACITY))[3]


@pytest.mark.parametrize("with_dst", [True, False], ids=["dst", "no_dst"])
def test_relocate_multiplicities_1_2_50_and_an_opaque_row(with_dst):
    """Rows drawn once, twice and 50 times in one call, in shuffled order; a row of opacity_logit = 30 (o = 1.0f in float32)
    drawn once: finite, its opacity clamped to 1 - 2^-23."""
    n = 257
    raw, mom = _relocate_scene(n, 2)
    raw["opacity_logit"][200] = F(30.0)
    sampled = np.random.default_rng(3).permutation(np.array([3] + [10] * 2 + [20] * 50 + [200]))
    dst = np.array([i for i in range(n) if i not in (3, 10, 20, 200)][:sampled.size][::-1]) if with_dst else None
    want = _relocate(raw, mom, sampled, dst, "multiplicities 1, 2, 50")
    assert [int(want["counts"][i]) for i in (3, 10, 20, 200)] == [1, 2, 50, 1] and want["counts"].sum() == 54
    assert want["want64"]["opacity_logit"][200] == math.log(R.TOP / (1.0 - R.TOP))
    assert (want["want64"]["opacity_logit"][[3, 10, 20]] < raw["opacity_logit"][[3, 10, 20]]).all()


@pytest.mark.parametrize("with_dst", [True, False], ids=["dst", "no_dst"])
def test_relocate_skips_and_counts_indices_out_of_range(with_dst):
    n = 130
    raw, mom = _relocate_scene(n, 4)
    sampled = [5, -1, 6, n, 5, 7, 2 ** 31 - 1, 8]
    dst = [100, 101, 102, 103, 104, n + 3, 106, -5] if with_dst else None
    want = _relocate(raw, mom, sampled, dst, "out of range")
    assert want["rejected"] == (5 if with_dst else 3)
    assert want["counts"].sum() == (3 if with_dst else 5) and want["counts"][5] == 2


@pytest.mark.parametrize("moments", [True, False], ids=["moments", "no_moments"])
def test_relocate_of_no_samples_touches_nothing(moments):
    raw, mom = _relocate_scene(65, 5)
    _relocate(raw, mom if moments else None, [], [], "m = 0")


# ---- 4. the module ----------------------------------------------------------------------------------------------------------
WITHOUT_STATE = "rotation"               # the optimiser has never stepped this parameter: it has no moments
SEED = 13


def _module_scene(n, seed, dead_share=0.3):
    raw, mom = _relocate_scene(n, seed)
    rng = np.random.default_rng(seed + 1)
    raw["opacity_logit"] = _logit(rng.uniform(0.2, 0.98, n))                 # (shared among a few copies it stays above min_opacity)
    dead = rng.random(n) < dead_share
    raw["opacity_logit"][dead] = (THRESHOLD - np.abs(rng.normal(size=int(dead.sum()))).astype(F)).astype(F)
    raw["opacity_logit"][np.nonzero(dead)[0][0]] = THRESHOLD                 # equal: dead
    return raw, {k: v for k, v in mom.items() if k != WITHOUT_STATE}


def _trainer(raw, moments, which):
    import torch
    from gsrast_amd.autograd import GaussianParams
    from gsrast_amd.optim import GaussianAdam
    params = GaussianParams.from_raw(*(raw[k] for k in R.RAW), device="cuda:0")
    groups = [{"params": [getattr(params, k)], "lr": 1e-3 * (i + 1)} for i, k in enumerate(R.RAW)]
    opt = GaussianAdam(groups) if which == "gaussian_adam" else torch.optim.Adam(groups)
    for k in moments:
        m, v = (torch.from_numpy(a.copy()).cuda() for a in moments[k])
        step = 7 if which == "gaussian_adam" else torch.tensor(7.0)
        opt.state[getattr(params, k)].update(step=step, exp_avg=m, exp_avg_sq=v)
    return params, opt


def _compare_module(params, opt, want, moments, hit, sampled, dst, n_old, what):
    """params and opt after a module call against the reference's result `want`, as _relocate compares."""
    host = lambda t: t.detach().cpu().numpy()
    n_new = want["raw"]["xyz"].shape[0]
    got_logit, got_ls = host(params.opacity_logit), host(params.log_scale)
    hit_new = np.concatenate([hit, np.zeros(n_new - n_old, bool)])
    _check_computed(got_logit, got_ls, None, want, hit_new, what)
    logit, ls = _adopt_computed(want, got_logit, got_ls, hit_new, sampled, dst, n_new)
    for k in R.RAW:
        w = {"opacity_logit": logit, "log_scale": ls}.get(k, want["raw"][k])
        assert host(getattr(params, k)).shape == w.shape and (_bits(host(getattr(params, k))) == _bits(w)).all(), (what, k)
        st = opt.state.get(getattr(params, k), {})
        if k in moments:
            assert float(st["step"]) == 7.0 and set(st) == {"step", "exp_avg", "exp_avg_sq"}
            for name, wm in zip(("exp_avg", "exp_avg_sq"), want["moments"][k]):
                assert (_bits(host(st[name])) == _bits(wm)).all(), (what, k, name)
        else:
            assert "exp_avg" not in st


@pytest.mark.parametrize("which", ["gaussian_adam", "torch_adam"])
def test_relocate_dead_is_the_reference_procedure_in_place(which):
    import torch
    from gsrast_amd import mcmc
    n = 1000
    raw, moments = _module_scene(n, 21)
    params, opt = _trainer(raw, moments, which)
    objects = [getattr(params, k) for k in R.RAW] + [opt.state[getattr(params, k)][m] for k in moments for m in ("exp_avg", "exp_avg_sq")]
    versions = [t._version for t in objects]
    # the reference procedure on the same u
    _, _, o = _activated(raw["opacity_logit"])
    dead_idx, weights, (dead, alive) = R.plan(raw["opacity_logit"], THRESHOLD, o)
    u = torch.rand(dead, dtype=torch.float64, generator=torch.Generator().manual_seed(SEED))
    sampled = mcmc.sample_rows(torch.from_numpy(weights), u).numpy()
    assert dead > 100 and alive > 100 and (weights[sampled] > 0).all() and np.unique(sampled).size < dead
    want = R.relocate(raw, moments, sampled, dead_idx, F(MIN_OPACITY), o)
    moved = mcmc.relocate_dead(params, opt, min_opacity=MIN_OPACITY, generator=torch.Generator().manual_seed(SEED))
    torch.cuda.synchronize()
    assert moved == dead
    now = [getattr(params, k) for k in R.RAW] + [opt.state[getattr(params, k)][m] for k in moments for m in ("exp_avg", "exp_avg_sq")]
    assert all(a is b for a, b in zip(objects, now)) and all(t._version > v for t, v in zip(now, versions))
    _compare_module(params, opt, want, moments, want["counts"] > 0, sampled, dead_idx, n, f"relocate_dead, {which}")
    assert not bool((params.opacity_logit <= float(THRESHOLD)).any())
    assert mcmc.relocate_dead(params, opt, generator=torch.Generator().manual_seed(SEED)) == 0      # nothing is dead now
    for k in R.RAW:
        getattr(params, k).grad = torch.ones_like(getattr(params, k))
    opt.step()                                                               # the optimiser goes on


def test_relocate_dead_with_nothing_alive_or_without_an_optimiser():
    import torch
    from gsrast_amd import mcmc
    raw, moments = _module_scene(300, 22)
    all_dead = dict(raw, opacity_logit=np.full(300, -9.0, F))
    params, opt = _trainer(all_dead, moments, "gaussian_adam")
    before = [getattr(params, k).detach().clone() for k in R.RAW]
    assert mcmc.relocate_dead(params, opt) == 0
    assert all(torch.equal(a, getattr(params, k).detach()) for a, k in zip(before, R.RAW))
    bare, _ = _trainer(raw, {}, "gaussian_adam")
    held, held_opt = _trainer(raw, moments, "gaussian_adam")
    gen = lambda: torch.Generator().manual_seed(SEED)
    assert mcmc.relocate_dead(bare, None, generator=gen()) == mcmc.relocate_dead(held, held_opt, generator=gen()) > 0
    assert all(torch.equal(getattr(bare, k), getattr(held, k)) for k in R.RAW)


@pytest.mark.parametrize("which", ["gaussian_adam", "torch_adam"])
def test_add_new_is_the_reference_procedure(which):
    import torch
    from gsrast_amd import mcmc
    n = 1000
    raw, moments = _module_scene(n, 23)
    params, opt = _trainer(raw, moments, which)
    old = [getattr(params, k) for k in R.RAW]
    lists = [g["params"] for g in opt.param_groups]
    _, _, o = _activated(raw["opacity_logit"])
    m = 50                                                                   # int(1.05 * 1000) - 1000
    u = torch.rand(m, dtype=torch.float64, generator=torch.Generator().manual_seed(SEED))
    sampled = mcmc.sample_rows(torch.from_numpy(o), u).numpy()               # the opacities of ALL rows, the dead ones too
    step2 = R.relocate(raw, moments, sampled, None, F(MIN_OPACITY), o)
    rows = np.concatenate([np.arange(n), sampled])
    new = np.arange(n + m) >= n
    want = dict(step2, raw={k: step2["raw"][k][rows] for k in R.RAW},
                moments={k: tuple(np.where(new.reshape((-1,) + (1,) * (a.ndim - 1)), F(0), a[rows]) for a in step2["moments"][k]) for k in moments},
                want64={k: np.concatenate([v, np.full(m, np.nan)]) for k, v in step2["want64"].items()})
    added = mcmc.add_new(params, opt, cap_max=5000, generator=torch.Generator().manual_seed(SEED))
    torch.cuda.synchronize()
    assert added == m and params.num_gaussians == n + m
    _compare_module(params, opt, want, moments, step2["counts"] > 0, sampled, n + np.arange(m), n, f"add_new, {which}")
    for i, k in enumerate(R.RAW):
        p = getattr(params, k)
        assert isinstance(p, torch.nn.Parameter) and p is not old[i] and p.requires_grad and p.grad is None
        assert opt.param_groups[i]["params"] is lists[i] and lists[i][0] is p and old[i] not in opt.state
    # the cap: 1050 -> 1060 of 1102, then 0 without replacing anything
    assert mcmc.add_new(params, opt, cap_max=1060) == 10 and params.num_gaussians == 1060
    held = [getattr(params, k) for k in R.RAW]
    versions = [p._version for p in held]
    assert mcmc.add_new(params, opt, cap_max=1060) == 0 and mcmc.add_new(params, opt, cap_max=500) == 0
    assert all(getattr(params, k) is p for k, p in zip(R.RAW, held)) and [p._version for p in held] == versions
    for k in R.RAW:
        getattr(params, k).grad = torch.ones_like(getattr(params, k))
    opt.step()


def test_refusals_leave_parameters_and_optimiser_untouched():
    import torch
    from gsrast_amd import mcmc
    from gsrast_amd.optim import GaussianAdam
    raw, moments = _module_scene(65, 24)
    calls = {"relocate_dead": lambda p, o: mcmc.relocate_dead(p, o), "add_new": lambda p, o: mcmc.add_new(p, o, cap_max=1000)}

    def refused(message, change):
        for name, call in calls.items():
            params, opt = _trainer(raw, moments, "gaussian_adam")
            opt = change(params, opt) or opt
            ids, values = [id(getattr(params, k)) for k in R.RAW], [getattr(params, k).detach().clone() for k in R.RAW]
            with pytest.raises(ValueError, match=name + ".*" + message):
                call(params, opt)
            assert ids == [id(getattr(params, k)) for k in R.RAW]
            assert all(torch.equal(v, getattr(params, k).detach()) for v, k in zip(values, R.RAW))

    def swap(make):
        def change(params, opt):
            old = params.rotation
            params.rotation = torch.nn.Parameter(make(old.detach()))
            opt.param_groups[3]["params"][0] = params.rotation
        return change

    def moment(alone=False, dtype=None):
        def change(params, opt):
            st = opt.state[params.log_scale]
            if alone:
                del st["exp_avg_sq"]
            else:
                st["exp_avg"] = st["exp_avg"].to(dtype)
        return change

    refused("does not hold shs", lambda p, o: GaussianAdam([p.xyz, p.opacity_logit, p.log_scale, p.rotation]))
    refused("exp_avg alone", moment(alone=True))
    refused("state exp_avg of log_scale is torch.float64", moment(dtype=torch.float64))
    refused("rotation is torch.float64", swap(lambda t: t.double()))
    refused("rotation is on cpu", swap(lambda t: t.cpu()))
    refused("rotation is not contiguous", swap(lambda t: torch.zeros((65, 8), device="cuda:0")[:, :4]))
    refused(r"rotation is \(64, 4\)", swap(lambda t: t[:64].clone()))
    params, opt = _trainer(raw, moments, "gaussian_adam")
    for bad in (0.0, 1.0):
        with pytest.raises(ValueError, match="min_opacity"):
            mcmc.relocate_dead(params, opt, min_opacity=bad)
        with pytest.raises(ValueError, match="min_opacity"):
            mcmc.add_new(params, opt, cap_max=1000, min_opacity=bad)


# ---- 5. a small training run ------------------------------------------------------------------------------------------------
def test_a_training_run_with_all_three_steps():
    """tests/test_gpu_densify.py's scene (168 Gaussians, eight behind the camera), a tenth of it dead at the start: render,
    loss plus the two regularisers, step, inject_noise; every four steps relocate_dead + add_new up to a cap of 1.15 N, through
    the same SplatRasterizer."""
    import torch
    from gsrast_amd import mcmc
    from gsrast_amd.autograd import GaussianParams, RadiiSlot, render
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer
    profile = "inria"
    cam, rast = _cam(1), _rasterizer()
    raw = {k: v.copy() for k, v in _raw_scene(profile).items()}
    make = lambda: GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major", device="cuda:0")
    with torch.no_grad():
        target = render(make(), rast, cam, **_kw(profile))[0]
    n0 = raw["xyz"].shape[0]
    cap = int(1.15 * n0)                                                     # (reached by the fourth growth of 5 %)
    expected = [min(cap, int(1.05 * n0))]
    for _ in range(3):
        expected.append(min(cap, int(1.05 * expected[-1])))
    raw["opacity_logit"][::10] = F(-8.0)
    params = make()
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    gen = torch.Generator().manual_seed(6)
    slot = RadiiSlot()
    sizes, relocated, losses = [], [], []
    for step in range(16):
        n = params.num_gaussians
        opt.zero_grad(set_to_none=True)
        color = render(params, rast, cam, radii_slot=slot, **_kw(profile))[0]
        reg = 0.01 * torch.sigmoid(params.opacity_logit).mean() + 0.01 * torch.exp(params.log_scale).mean()
        loss = (color - target).abs().mean() + reg
        losses.append(float(loss.detach()))
        loss.backward()
        assert rast.num_gaussians == n and all(getattr(params, k).grad.shape[0] == n for k in RAW)
        opt.step()
        mcmc.inject_noise(params, rates["xyz"] * 5e5, generator=gen)
        if step % 4 == 3:
            relocated.append(mcmc.relocate_dead(params, opt, min_opacity=MIN_OPACITY, generator=gen))
            assert not bool((params.opacity_logit <= float(THRESHOLD)).any())            # nothing at or below the threshold now
            mcmc.add_new(params, opt, cap_max=cap, min_opacity=MIN_OPACITY, generator=gen)
            sizes.append(params.num_gaussians)
    torch.cuda.synchronize()
    print(f"[mcmc training] {n0} Gaussians -> {sizes}; relocated {relocated}; loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert relocated[0] >= len(range(0, n0, 10)) and sizes == expected and sizes[-1] == cap
    assert all(np.isfinite(losses)) and all(bool(torch.isfinite(getattr(params, k)).all()) for k in RAW)
    assert all(getattr(params, k).shape[0] == cap for k in RAW)
