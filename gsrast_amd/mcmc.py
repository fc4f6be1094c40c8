"""3DGS-MCMC (Kheradmand et al. 2024) over GaussianParams and an Adam: a fixed budget of Gaussians instead of clone / split /
prune, in HIP (gsr_mcmc_noise / _plan / _relocate, csrc/mcmc.hip; include/gsrast_amd_mcmc.h states the arithmetic).

    for step in range(...):
        color, _, _ = render(params, rast, cam)
        reg = lam_o * torch.sigmoid(params.opacity_logit).mean() + lam_s * torch.exp(params.log_scale).mean()
        (photometric_loss(color, target) + reg).backward()
        opt.step()
        inject_noise(params, xyz_lr * noise_lr)                    # one launch, every step
        if step % 100 == 0:
            relocate_dead(params, opt)                             # dead Gaussians move onto live ones, N unchanged
            add_new(params, opt, cap_max=1_000_000)                # N grows by 5 % up to the cap

relocate_dead works in place: parameters and optimiser state stay the same objects. add_new replaces the five nn.Parameters
the way densify_and_prune does (and only when it adds a row). relocate_dead synchronises once, the others not at all.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _capi
from .autograd import GaussianParams
from .densify import RAW, _refuse, gather_rows, held_arrays, replace_parameters


def _bump(*tensors) -> None:
    # the kernels wrote through raw pointers: autograd's saved-tensor check and whatever keys on ._version must see the write
    for t in tensors:
        torch.autograd.graph.increment_version(t)


def inject_noise(params: GaussianParams, scaler: float, *, generator=None, noise: "torch.Tensor | None" = None) -> None:
    """xyz += covariance x (noise x gate(opacity) x scaler), in place, one launch on the current stream, no synchronisation.
    scaler: learning rate x noise_lr (a double, rounded to float once). noise: f32[N, 3] standard normal on the parameters'
    device; drawn with torch.randn((N, 3), generator=generator) unless given. The gate is sigmoid(100 ((1 - o) - 0.995)): a
    Gaussian of opacity above 0.005 hardly moves. params.xyz's version is bumped (a graph that saved it refuses to run
    backward afterwards). Raises ValueError before the launch for arrays the kernel cannot take."""
    xyz, logit, ls, rot = params.xyz, params.opacity_logit, params.log_scale, params.rotation
    n, dev = int(xyz.shape[0]), xyz.device
    if not xyz.is_cuda:
        raise ValueError(f"inject_noise: the parameters are on {dev}, not on a GPU")
    for t, name, shape in ((xyz, "xyz", (n, 3)), (logit, "opacity_logit", (n,)), (ls, "log_scale", (n, 3)), (rot, "rotation", (n, 4))):
        _refuse(t, name, shape, dev, "inject_noise")
    if noise is None:
        noise_dev = generator.device if generator is not None else dev
        noise = torch.randn((n, 3), generator=generator, dtype=torch.float32, device=noise_dev).to(dev)
    else:
        if not isinstance(noise, torch.Tensor):
            raise ValueError(f"inject_noise: noise is a {type(noise).__name__}, not a tensor")
        _refuse(noise, "noise", (n, 3), dev, "inject_noise")
    if n == 0:
        return
    a = _capi.McmcNoiseArgs()
    a.struct_size, a.scaler, a.n = C.sizeof(_capi.McmcNoiseArgs), float(scaler), n
    a.xyz, a.opacity_logit, a.log_scale, a.rotation = xyz.data_ptr(), logit.data_ptr(), ls.data_ptr(), rot.data_ptr()
    a.noise, a.stream = noise.data_ptr(), _capi.stream(dev)
    with torch.no_grad():
        _capi.call("gsr_mcmc_noise", C.byref(a), device=dev)
        _bump(xyz)


def sample_rows(weights: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """Rows drawn in proportion to `weights` (>= 0, any float dtype, any device) by inverting their cumulative sum in
    double at the uniform numbers u in [0, 1): int64[len(u)]. Unlike torch.multinomial the number of rows has no limit. A row
    of weight 0 is never returned — not for u = 0 (the search is for the first cdf entry ABOVE the target), and not where
    rounding carries u x total up to the total (the last row of non-zero weight is returned then). ValueError when every
    weight is 0 (or there is none)."""
    if weights.dim() != 1 or u.dim() != 1:
        raise ValueError(f"sample_rows: weights {tuple(weights.shape)} and u {tuple(u.shape)} must both have one dimension")
    cdf = torch.cumsum(weights.double(), 0)
    if cdf.numel() == 0 or not bool(cdf[-1] > 0):
        raise ValueError("sample_rows: every weight is 0")
    return _invert(cdf, u)


def _invert(cdf: torch.Tensor, u: torch.Tensor) -> torch.Tensor:
    """sample_rows behind its check (which synchronises): the callers below know that a weight is above 0."""
    idx = torch.searchsorted(cdf, u.double().to(cdf.device) * cdf[-1], right=True)
    # cdf[last] == cdf[-1] for the first time at the last row of non-zero weight
    last = torch.searchsorted(cdf, cdf[-1:], right=False)
    return torch.minimum(idx, last)


def _relocate(old, held, n: int, dev, sampled: torch.Tensor, dst: "torch.Tensor | None", min_opacity: float) -> None:
    m = int(sampled.shape[0])
    temp = torch.empty(int(_capi.lib().gsr_mcmc_relocate_temp_bytes(n)), dtype=torch.uint8, device=dev)
    a = _capi.McmcRelocateArgs()
    a.struct_size, a.min_opacity, a.n, a.m = C.sizeof(_capi.McmcRelocateArgs), float(min_opacity), n, m
    a.sampled, a.dst = sampled.data_ptr(), dst.data_ptr() if dst is not None else None
    a.temp, a.stream = temp.data_ptr(), _capi.stream(dev)
    for k in RAW:
        arr = getattr(a, k)
        arr.param = old[k].data_ptr()
        if k in held:
            arr.exp_avg, arr.exp_avg_sq = (t.data_ptr() for t in held[k])
    with torch.no_grad():
        _capi.call("gsr_mcmc_relocate", C.byref(a), device=dev)
        _bump(*old.values(), *(t for pair in held.values() for t in pair))


def _uniform(count: int, generator, dev) -> torch.Tensor:
    u_dev = generator.device if generator is not None else dev
    return torch.rand(count, dtype=torch.float64, generator=generator, device=u_dev).to(dev)


def _check_min_opacity(where: str, min_opacity: float) -> None:
    if not 0.0 < min_opacity < 1.0:
        raise ValueError(f"{where}: min_opacity must lie in (0, 1)")


def _plan(opacity_logit, n: int, dev, logit_min_opacity: float):
    """gsr_mcmc_plan -> (dead_idx i32[n], weights f32[n], counts i32[2]) on the device, not synchronised."""
    temp = torch.empty(int(_capi.lib().gsr_mcmc_plan_temp_bytes(n)), dtype=torch.uint8, device=dev)
    dead_idx, counts = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(2, dtype=torch.int32, device=dev)
    weights = torch.empty(n, dtype=torch.float32, device=dev)
    _capi.call("gsr_mcmc_plan", n, opacity_logit.data_ptr(), logit_min_opacity, temp.data_ptr(), dead_idx.data_ptr(), weights.data_ptr(),
               counts.data_ptr(), _capi.stream(dev), device=dev)
    return dead_idx, weights, counts


def relocate_dead(params: GaussianParams, opt, *, min_opacity: float = 0.005, generator=None) -> int:
    """Every dead Gaussian (opacity_logit <= logit(min_opacity), compared on the raw values) becomes a copy of a live one
    drawn in proportion to its opacity (torch.rand(dead, dtype=float64, generator=generator), inverted as by sample_rows); a live
    one drawn c times shares its opacity with its c copies and shrinks so that the picture stays the same
    (gsr_mcmc_relocate). Both Adam moments of sources and destinations become 0. All in place: the five nn.Parameters
    and the optimiser's state tensors stay the same objects, their versions are bumped. opt: a GaussianAdam or
    torch.optim.Adam that holds all five, or None. One synchronisation (the two counts). Returns the number of Gaussians
    relocated: 0, without another launch, when none is dead or none alive.

    Raises ValueError before anything is launched: as densify_and_prune."""
    old, n, dev, held = held_arrays(params, opt, "relocate_dead")
    _check_min_opacity("relocate_dead", min_opacity)
    if n == 0:
        return 0
    dead_idx, weights, counts = _plan(old["opacity_logit"], n, dev, math.log(min_opacity / (1.0 - min_opacity)))
    dead, alive = (int(c) for c in counts.tolist())                                    # (the one synchronisation)
    if dead == 0 or alive == 0:
        return 0
    sampled = _invert(torch.cumsum(weights.double(), 0), _uniform(dead, generator, dev)).to(torch.int32)
    _relocate(old, held, n, dev, sampled, dead_idx, min_opacity)
    return dead


def add_new(params: GaussianParams, opt, *, cap_max: int, growth: float = 0.05, min_opacity: float = 0.005, generator=None) -> int:
    """N grows to min(cap_max, int((1 + growth) N)): the new Gaussians are copies of rows drawn in proportion to the
    opacities of ALL rows (as upstream; gsr_mcmc_plan with no threshold forms them), the sources updated as in relocate_dead (gsr_mcmc_relocate without destinations),
    then all rows gathered into arrays of the new count by gsr_densify_apply (a new row copies its updated source; its
    moments are 0). The five nn.Parameters are replaced and the optimiser re-keyed as by densify_and_prune — unless no
    row is added: then nothing is launched and nothing replaced. No synchronisation (N is known). growth <= 1. Returns
    the number of rows added.

    Raises ValueError before anything is launched: as densify_and_prune."""
    old, n, dev, held = held_arrays(params, opt, "add_new")
    _check_min_opacity("add_new", min_opacity)
    if not 0.0 <= growth <= 1.0:
        raise ValueError(f"add_new: a growth of {growth}")
    m = max(0, min(int(cap_max), int((1.0 + growth) * n)) - n)
    if m == 0:
        return 0
    _, weights, _ = _plan(old["opacity_logit"], n, dev, -math.inf)                     # (no row is dead: the opacity of every row)
    sampled = _invert(torch.cumsum(weights.double(), 0), _uniform(m, generator, dev)).to(torch.int32)
    _relocate(old, held, n, dev, sampled, None, min_opacity)
    src_of = torch.cat([torch.arange(n, dtype=torch.int32, device=dev), sampled])
    fresh, fresh_moments = gather_rows(old, held, n, (n, m, 0, n + m), src_of, None, 0.0, dev)
    replace_parameters(params, opt, old, held, fresh, fresh_moments)
    return m
