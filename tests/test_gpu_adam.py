"""GPU: gsr_adam_step through gsrast_amd.optim.GaussianAdam — bit for bit against the float32 reference (tests/adam_ref.py)
over every row width, wave edge and visibility pattern, with NaN gradients in culled rows and sentinels around every array;
dense against torch.optim.Adam; parameter groups; the version counter and a stale graph; a short sparse training run; and
a densification-style edit of the optimiser's state."""
import re

import numpy as np
import pytest

import adam_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 7, 48)             # scalar, scalar, LDS triples, float4, scalar in partial passes, float4 in 16-row units
SENTINEL = -7.0
GAP = 64                                 # sentinel floats on both sides of every array
# a group per width: the six scalars are per array
GROUPS = {1: dict(lr=2.5e-2, betas=(0.9, 0.999), eps=1e-8), 2: dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-6),
          3: dict(lr=1.6e-4, betas=(0.9, 0.999), eps=1e-15), 4: dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-15),
          7: dict(lr=5e-3, betas=(0.5, 0.9), eps=1e-8), 48: dict(lr=2.5e-3, betas=(0.9, 0.999), eps=1e-15)}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _visibility(kind, n, rng):
    """i32[n] or None. Culled rows carry zeros and negative values."""
    if kind == "dense":
        return None
    culled = np.where(np.arange(n) % 3 == 0, -1, 0).astype(np.int32)
    if kind == "all":
        on = np.ones(n, bool)
    elif kind == "none":
        on = np.zeros(n, bool)
    elif kind == "alternating":
        on = np.arange(n) % 2 == 1
    elif kind == "wave_culled":                      # rows 64..127: one whole wave of an array of up to four floats per row
        on = ~((np.arange(n) >= 64) & (np.arange(n) < 128))
    elif kind == "last_row":                         # only the last row (of a partial wave where n is no multiple of 64)
        on = np.arange(n) == n - 1
    else:
        assert kind == "random"
        on = rng.random(n) < 0.52
    return np.where(on, rng.integers(1, 200, n), culled).astype(np.int32)


def _gradient(rng, shape, visible):
    """Magnitudes 10^-3 .. 10 (nothing denormal is met on the way), NaN in the rows the step must not read."""
    g = np.asarray(rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-3, 1, shape), dtype=np.float32)
    if visible is not None:
        g[visible <= 0] = np.nan
    return g


class _Arena:
    """One device buffer filled with a sentinel; p, g, m, v of every width are 16-byte-aligned slices of it, GAP sentinel
    floats on both sides of each. `host` is what the buffer is expected to hold."""

    def __init__(self, n, widths, rng):
        import torch
        self.n, self.slices, at = n, {}, GAP
        for w in widths:
            for name in "pgmv":
                self.slices[w, name] = slice(at, at + n * w)
                at += (n * w + 3) // 4 * 4 + GAP
        self.host = np.full(at, SENTINEL, np.float32)
        for w in widths:
            self.host[self.slices[w, "p"]] = rng.normal(size=n * w)
            self.host[self.slices[w, "m"]] = 0.1 * rng.normal(size=n * w)
            self.host[self.slices[w, "v"]] = 10.0 ** rng.uniform(-4, 0, n * w)
        self.dev = torch.from_numpy(self.host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def tensor(self, w, name):
        t = self.dev[self.slices[w, name]].view(self.n, w) if w > 1 else self.dev[self.slices[w, name]]     # (width 1: [N], as the opacity)
        assert t.data_ptr() % 16 == 0 and t.is_contiguous()
        return t

    def array(self, w, name):
        return self.host[self.slices[w, name]].reshape((self.n, w) if w > 1 else (self.n,))

    def put(self, w, name, a):
        import torch
        self.host[self.slices[w, name]] = a.reshape(-1)
        self.dev[self.slices[w, name]] = torch.from_numpy(a.reshape(-1)).cuda()

    def mismatches(self):
        """Where the device buffer differs from `host`, bit for bit: the names of the arrays, or 'sentinel'."""
        import torch
        torch.cuda.synchronize()
        diff = _bits(self.dev.cpu().numpy()) != _bits(self.host)
        where = []
        for (w, name), q in self.slices.items():
            if diff[q].any():
                where.append(f"{name}[width {w}] rows {sorted(set(np.nonzero(diff[q])[0] // w))[:8]}")
                diff[q] = False
        if diff.any():
            where.append(f"sentinel at {np.nonzero(diff)[0][:8].tolist()}")
        return where


def _optimizer(arena, widths, step=0):
    """A GaussianAdam over the arena's parameters, one group per width, the moments the arena's slices."""
    from gsrast_amd.optim import GaussianAdam
    params = {w: arena.tensor(w, "p").requires_grad_() for w in widths}
    opt = GaussianAdam([dict(params=[params[w]], **GROUPS[w]) for w in widths])
    for w in widths:
        params[w].grad = arena.tensor(w, "g")
        opt.state[params[w]].update(step=step, exp_avg=arena.tensor(w, "m"), exp_avg_sq=arena.tensor(w, "v"))
    return opt, params


def _reference_step(arena, widths, t, visible):
    for w in widths:
        kw = GROUPS[w]
        p, m, v = R.step32(arena.array(w, "p"), arena.array(w, "g"), arena.array(w, "m"), arena.array(w, "v"), t,
                           lr=kw["lr"], betas=kw["betas"], eps=kw["eps"], visible=visible)
        for name, a in zip("pmv", (p, m, v)):
            arena.host[arena.slices[w, name]] = a.reshape(-1)


# ---- 1. bit for bit against step32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["dense", "all", "none", "alternating", "wave_culled", "last_row", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_step_is_the_float32_reference_bit_for_bit(n, kind):
    """All six widths in one call (one launch: every array's units behind the other's), each with its own scalars. Three
    steps with fresh gradients, then one at step count 1001. After every step the WHOLE buffer is compared with what the
    reference expects: visible rows updated, culled rows, gradients and sentinels as they were."""
    import torch
    rng = np.random.default_rng(1000 * n + len(kind))
    arena = _Arena(n, WIDTHS, rng)
    opt, params = _optimizer(arena, WIDTHS)
    for t in (1, 2, 3, 1001):
        visible = _visibility(kind, n, rng)
        if t == 1001:
            for p in params.values():
                opt.state[p]["step"] = torch.tensor(1000.0)             # (as a torch.optim.Adam state dict carries it)
        for w in WIDTHS:
            arena.put(w, "g", _gradient(rng, (n, w), visible))
        before = arena.host.copy()
        opt.step(None if visible is None else torch.from_numpy(visible).cuda())
        _reference_step(arena, WIDTHS, t, visible)
        assert arena.mismatches() == [], (t, kind)
        assert all(int(opt.state[p]["step"]) == t for p in params.values())
        changed = _bits(before) != _bits(arena.host)
        if visible is None or (visible > 0).any():
            assert changed.any()                                        # (the reference itself moved something)
        else:
            assert not changed.any()
    # a bool mask is the same call
    if kind == "random":
        visible = _visibility(kind, n, rng)
        for w in WIDTHS:
            arena.put(w, "g", _gradient(rng, (n, w), visible))
        opt.step(torch.from_numpy(visible > 0).cuda())
        _reference_step(arena, WIDTHS, 1002, visible)
        assert arena.mismatches() == []


@pytest.mark.parametrize("w", WIDTHS)
def test_one_array_alone_gives_the_same_bits(w):
    """One launch per array instead of one for all: the same reference (the result does not depend on the launch shape)."""
    import torch
    n = 257
    rng = np.random.default_rng(70 + w)
    arena = _Arena(n, (w,), rng)
    opt, _ = _optimizer(arena, (w,))
    for t in (1, 2):
        visible = _visibility("random", n, rng)
        arena.put(w, "g", _gradient(rng, (n, w), visible))
        opt.step(torch.from_numpy(visible).cuda())
        _reference_step(arena, (w,), t, visible)
        assert arena.mismatches() == []


# ---- 2. dense against torch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 48])
def test_dense_steps_are_as_close_to_float64_as_torchs(w):
    """Dense GaussianAdam and torch.optim.Adam from the same values with the same gradients, five steps; each against
    step64: ours errs at most twice as much as torch's (absolute for p, relative for the moments)."""
    import torch
    from gsrast_amd.optim import GaussianAdam
    n, steps, lr = 1000, 5, 1e-2
    rng = np.random.default_rng(300 + w)
    p0 = rng.normal(size=(n, w)).astype(np.float32)
    mag = 10.0 ** rng.uniform(-3, 1, (n, w))
    grads = [(rng.normal(size=(n, w)) * mag).astype(np.float32) for _ in range(steps)]
    ours, theirs = (torch.nn.Parameter(torch.from_numpy(p0.copy()).cuda()) for _ in range(2))
    opt_ours, opt_theirs = GaussianAdam([ours], lr=lr), torch.optim.Adam([theirs], lr=lr)
    p64, m64, v64 = p0.astype(np.float64), np.zeros((n, w)), np.zeros((n, w))
    for t, g in enumerate(grads, 1):
        ours.grad, theirs.grad = torch.from_numpy(g).cuda(), torch.from_numpy(g).cuda()
        opt_ours.step()
        opt_theirs.step()
        p64, m64, v64 = R.step64(p64, g, m64, v64, t, lr=lr)
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy().astype(np.float64)
    so, st = opt_ours.state[ours], opt_theirs.state[theirs]
    assert float(np.abs(p64 - p0).max()) > 1e-2 and (m64 != 0).all()
    for name, a, b, want, relative in (("p", host(ours), host(theirs), p64, False),
                                       ("exp_avg", host(so["exp_avg"]), host(st["exp_avg"]), m64, True),
                                       ("exp_avg_sq", host(so["exp_avg_sq"]), host(st["exp_avg_sq"]), v64, True)):
        scale = np.abs(want) if relative else 1.0
        e_ours, e_torch = float((np.abs(a - want) / scale).max()), float((np.abs(b - want) / scale).max())
        print(f"[adam dense] width {w} {name}: ours {e_ours:.3e}, torch {e_torch:.3e}")
        assert e_torch > 0 and e_ours <= 2.0 * e_torch, name


# ---- 3. groups --------------------------------------------------------------------------------------------------------------
def test_groups_of_other_rates_and_sizes_and_a_parameter_without_gradient():
    """Three groups with their own lr, betas and eps; tensors of different row counts under visibility=None (a call per
    row count, at most eight arrays per launch: twelve share one count); a learning rate changed between steps; a
    parameter without a gradient keeps its state and step count."""
    import torch
    from gsrast_amd.optim import GaussianAdam
    rng = np.random.default_rng(5)
    shapes = {"a": [(100, 3), (100,), ()], "b": [(37, 48), (37, 4), (37, 2, 2)], "c": [(5, 7)] + [(50, 2)] * 12}
    settings = {"a": dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8), "b": dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-15),
                "c": dict(lr=5e-3, betas=(0.5, 0.9), eps=1e-6)}
    new = lambda shape: torch.nn.Parameter(torch.from_numpy(rng.normal(size=shape).astype(np.float32)).cuda())
    groups = {k: [new(s) for s in v] for k, v in shapes.items()}
    idle = new((100, 3))
    opt = GaussianAdam([dict(params=groups[k] + ([idle] if k == "a" else []), **settings[k]) for k in "abc"])
    opt.state[idle].update(step=7, exp_avg=torch.full((100, 3), 0.5).cuda(), exp_avg_sq=torch.full((100, 3), 0.25).cuda())
    idle_before = idle.detach().clone()
    want = {p: (p.detach().cpu().numpy(), np.zeros(tuple(p.shape), np.float32), np.zeros(tuple(p.shape), np.float32))
            for k in "abc" for p in groups[k]}
    for t in (1, 2, 3):
        if t == 2:
            opt.param_groups[1]["lr"] = settings["b"]["lr"] = 4e-4          # (a scheduler's write)
        for k in "abc":
            for p in groups[k]:
                g = _gradient(rng, tuple(p.shape), None)
                p.grad = torch.from_numpy(g).cuda().reshape(p.shape)
                rows = lambda a: a.reshape(max(1, a.shape[0] if a.ndim else 1), -1)
                pw, mw, vw = want[p]
                out = R.step32(rows(pw), rows(g), rows(mw), rows(vw), t, **settings[k])
                want[p] = tuple(a.reshape(pw.shape) for a in out)
        opt.step()
        torch.cuda.synchronize()
        for p, (pw, mw, vw) in want.items():
            st = opt.state[p]
            assert st["step"] == t
            for name, got, w in (("p", p, pw), ("exp_avg", st["exp_avg"], mw), ("exp_avg_sq", st["exp_avg_sq"], vw)):
                assert (_bits(got.detach().cpu().numpy()) == _bits(w)).all(), (tuple(p.shape), name, t)
    st = opt.state[idle]
    assert st["step"] == 7 and idle._version == 0 and torch.equal(idle.detach(), idle_before)
    assert bool((st["exp_avg"] == 0.5).all()) and bool((st["exp_avg_sq"] == 0.25).all())
    # with a visibility array every parameter of the call has its rows
    with pytest.raises(ValueError, match="visibility has 100 rows"):
        opt.step(torch.ones(100, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="not i32"):
        opt.step(torch.ones(100, dtype=torch.int64).cuda())
    assert all(opt.state[p]["step"] == 3 for p in want)


# ---- 4. the version counter and a stale graph -------------------------------------------------------------------------------
def test_a_step_is_an_in_place_write_autograd_sees():
    import torch
    from gsrast_amd.autograd import render
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_autograd import DRAW, RAW, _cam, _kw, _params, _rasterizer, _weights
    profile = "gscuda"
    wt = _weights()[0]
    messages = {}
    for name in ("torch", "ours"):
        params, rast = _params(profile), _rasterizer()
        make = torch.optim.Adam if name == "torch" else GaussianAdam
        opt = make(list(params.parameters()), lr=1e-3)
        (wt * render(params, rast, _cam(1), **_kw(profile), **DRAW)[0]).sum().backward()
        versions = [[getattr(params, k)._version for k in RAW]]
        stale = (wt * render(params, rast, _cam(1), **_kw(profile), **DRAW)[0]).sum()        # a graph built before the step ...
        opt.step()
        versions.append([getattr(params, k)._version for k in RAW])
        opt.step()
        versions.append([getattr(params, k)._version for k in RAW])
        assert all(a < b < c for a, b, c in zip(*versions)), (name, versions)               # p._version grows with every step
        grads = [getattr(params, k).grad.clone() for k in RAW]
        with pytest.raises(RuntimeError, match="modified by an inplace operation") as info:  # ... is refused in backward()
            stale.backward()
        messages[name] = re.sub(r"version \d+", "version N", str(info.value))
        torch.cuda.synchronize()
        assert all(torch.equal(g, getattr(params, k).grad) for g, k in zip(grads, RAW))     # (and has accumulated nothing)
    # the same check trips on the same tensor
    assert messages["ours"] == messages["torch"]


# ---- 5. training ------------------------------------------------------------------------------------------------------------
EXTRA = 8


def _train_sparse(steps=20):
    """tests/test_gpu_autograd.py's training run with GaussianAdam fed the frames' radii, the scene with eight Gaussians
    behind the camera added. -> losses, the final five arrays, the initial five arrays, seen-in-some-step i32[N]"""
    import torch
    from gsrast_amd.autograd import GaussianParams, RadiiSlot, render
    from gsrast_amd.optim import GaussianAdam
    from test_gpu_autograd import RAW, _cam, _kw, _raw_scene, _rasterizer
    profile = "inria"
    cam, rast = _cam(1), _rasterizer()
    raw = {k: v.copy() for k, v in _raw_scene(profile).items()}
    rng = np.random.default_rng(9)
    eye = np.asarray(cam.cam_pos, np.float64).reshape(-1)[:3]
    back = eye / np.linalg.norm(eye)                                            # (the camera looks at the origin)
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
    start = [getattr(params, k).detach().clone() for k in RAW]
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    slot = RadiiSlot()
    seen = torch.zeros(params.num_gaussians, dtype=torch.int32, device="cuda:0")
    losses = []
    for _ in range(steps + 1):
        opt.zero_grad(set_to_none=True)
        loss = (render(params, rast, cam, radii_slot=slot, **_kw(profile))[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        if len(losses) <= steps:
            loss.backward()
            assert slot.radii.dtype == torch.int32 and tuple(slot.radii.shape) == (params.num_gaussians,)
            seen = torch.maximum(seen, slot.radii)
            opt.step(slot.radii)
    return losses, [getattr(params, k).detach().clone() for k in RAW], start, seen.cpu().numpy()


def test_twenty_sparse_steps_lower_the_loss_and_leave_unseen_gaussians_alone():
    from test_gpu_autograd import N, _same_bits
    losses, end, start, seen = _train_sparse()
    print(f"[sparse training] L1 loss {losses[0]:.6f} -> {losses[-1]:.6f}, {(seen > 0).sum()} of {seen.size} Gaussians seen")
    assert seen.size == N + EXTRA == 168 and (seen > 0).sum() >= seen.size / 2
    assert all(np.isfinite(losses)) and losses[0] > 0 and losses[-1] < losses[0]
    assert (seen[N:] <= 0).all()                                                # the eight behind the camera: never seen
    for a, b in zip(end, start):
        assert _same_bits(a[N:], b[N:])                                         # ... and end with their initial bits
        assert not _same_bits(a[:N], b[:N])
        unseen = seen <= 0                                                      # (a bool mask indexes a tensor as it does an array)
        assert _same_bits(a[unseen], b[unseen])
    losses2, end2, _, seen2 = _train_sparse()
    assert losses2 == losses and (seen2 == seen).all()
    for a, b in zip(end, end2):
        assert _same_bits(a, b)


# ---- 6. densification-style surgery -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [3, 48])
def test_a_longer_parameter_with_concatenated_moments_continues(w):
    """What a trainer's densification does to an Adam: the parameter replaced by one 37 rows longer, its state moved over
    with zeros appended to both moments. The next step continues the old rows as if nothing had happened."""
    import torch
    from gsrast_amd.optim import GaussianAdam
    n, more = 100, 37
    rng = np.random.default_rng(600 + w)
    kw = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-15)
    up = lambda a: torch.from_numpy(a).cuda()
    pw = rng.normal(size=(n, w)).astype(np.float32)
    mw, vw = np.zeros((n, w), np.float32), np.zeros((n, w), np.float32)
    p = torch.nn.Parameter(up(pw))
    opt = GaussianAdam([p], **kw)
    for t in (1, 2):
        visible = _visibility("random", n, rng)
        g = _gradient(rng, (n, w), visible)
        p.grad = up(g)
        opt.step(up(visible))
        pw, mw, vw = R.step32(pw, g, mw, vw, t, visible=visible, **kw)
    # the surgery (the upstream trainer's cat_tensors_to_optimizer)
    added = rng.normal(size=(more, w)).astype(np.float32)
    stored = opt.state.pop(p)
    stored["exp_avg"] = torch.cat([stored["exp_avg"], torch.zeros((more, w), device="cuda:0")])
    stored["exp_avg_sq"] = torch.cat([stored["exp_avg_sq"], torch.zeros((more, w), device="cuda:0")])
    longer = torch.nn.Parameter(torch.cat([p.detach(), up(added)]))
    opt.param_groups[0]["params"][0] = longer
    opt.state[longer] = stored
    pw, mw, vw = np.concatenate([pw, added]), np.concatenate([mw, np.zeros_like(added)]), np.concatenate([vw, np.zeros_like(added)])
    visible = _visibility("random", n + more, rng)
    g = _gradient(rng, (n + more, w), visible)
    longer.grad = up(g)
    opt.step(up(visible))
    pw, mw, vw = R.step32(pw, g, mw, vw, 3, visible=visible, **kw)
    torch.cuda.synchronize()
    st = opt.state[longer]
    assert st["step"] == 3 and (visible[:n] > 0).any() and (visible[n:] > 0).any()
    for name, got, want in (("p", longer, pw), ("exp_avg", st["exp_avg"], mw), ("exp_avg_sq", st["exp_avg_sq"], vw)):
        assert (_bits(got.detach().cpu().numpy()) == _bits(want)).all(), name
