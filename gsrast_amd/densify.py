"""Adaptive density control: the clone / split / prune of a 3DGS trainer over GaussianParams and a GaussianAdam, in HIP
(gsr_densify_accumulate / _plan / _apply, csrc/densify.hip; include/gsrast_amd.h states the classes and the arithmetic).

    slot, stats = FrameSlot(), DensityStats(params.num_gaussians, dev)
    for step in range(...):
        color, _, _ = render(params, rast, cam, radii_slot=slot)
        photometric_loss(color, target).backward()
        opt.step(slot.radii)
        stats.update(slot, rast.width, rast.height)              # one launch: |dL_dmean2D| in NDC, seen count, largest radius
        if step % 100 == 0:
            densify_and_prune(params, opt, stats, extent=scene_extent, max_screen_size=20)
        if step % 3000 == 0:
            reset_opacity(params, opt)

densify_and_prune replaces the five nn.Parameters of `params` by new ones of the new row count and moves the optimiser's
state along: it synchronises once, to read the four counts the new arrays are sized by.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _capi
from .autograd import FrameSlot, GaussianParams

RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
ROW_FLOATS = {"xyz": 3, "opacity_logit": 1, "log_scale": 3, "rotation": 4, "shs": 48}
MOMENTS = ("exp_avg", "exp_avg_sq")


def plan_scalars(max_grad: float, min_opacity: float, extent: float, percent_dense: float):
    """The five floats gsr_densify_plan takes, computed in double; ctypes rounds each to float once.
    (max_grad, log_dense, logit_min_opacity, log_world, log_shrink)"""
    return (max_grad, math.log(percent_dense * extent), math.log(min_opacity / (1.0 - min_opacity)), math.log(0.1 * extent),
            math.log(0.8 * 2))


class DensityStats:
    """What the decision rests on, per Gaussian, since the last densification: grad_accum f32[N] (the sum over the frames
    that saw it of |dL_dmean2D| in upstream's NDC convention), denom i32[N] (how many frames saw it) and max_radii i32[N]
    (its largest screen radius in them)."""

    def __init__(self, n: int, device):
        self.device = torch.device(device)
        self.reset(n)

    def reset(self, n: int) -> None:
        """Zeros at a new row count."""
        self.grad_accum = torch.zeros(int(n), dtype=torch.float32, device=self.device)
        self.denom = torch.zeros(int(n), dtype=torch.int32, device=self.device)
        self.max_radii = torch.zeros(int(n), dtype=torch.int32, device=self.device)

    @property
    def num_gaussians(self) -> int:
        return int(self.grad_accum.shape[0])

    def update(self, slot: FrameSlot, width: int, height: int, absgrad: bool = False) -> None:
        """Adds the frame `slot` carries (after its backward). One launch on the current stream, no synchronisation; a
        Gaussian the frame culled keeps its three statistics and its gradient is not read.
        absgrad=True: AbsGS's score — slot.abs_dL_dmean2D (a FrameSlot(absgrad=True)) is accumulated in place of dL_dmean2D,
        by the same kernel; ValueError if the slot holds none. grad_accum is then on another scale: see densify_and_prune."""
        n = self.num_gaussians
        radii, grad = slot.radii, getattr(slot, "abs_dL_dmean2D" if absgrad else "dL_dmean2D", None)
        if absgrad and grad is None:
            raise ValueError("DensityStats.update(absgrad=True): the slot holds no abs_dL_dmean2D (a FrameSlot(absgrad=True) "
                             "after render() and backward())")
        if radii is None or grad is None:
            raise ValueError("DensityStats.update: the slot holds no frame (a FrameSlot after render() and backward())")
        if (radii.dtype != torch.int32 or tuple(radii.shape) != (n,) or grad.dtype != torch.float32 or tuple(grad.shape) != (n, 2)
                or radii.device != self.device or grad.device != self.device or not radii.is_contiguous() or not grad.is_contiguous()):
            raise ValueError(f"DensityStats.update: the statistics have {n} rows on {self.device}; the slot's radii are "
                             f"{radii.dtype} {tuple(radii.shape)} on {radii.device}, its dL_dmean2D {grad.dtype} {tuple(grad.shape)}")
        _capi.call("gsr_densify_accumulate", n, grad.data_ptr(), radii.data_ptr(), 0.5 * width, 0.5 * height, self.grad_accum.data_ptr(),
                   self.denom.data_ptr(), self.max_radii.data_ptr(), _capi.stream(self.device), device=self.device)


def _refuse(t: torch.Tensor, name: str, shape, dev, where: str = "densify_and_prune") -> None:
    if t.dtype != torch.float32:
        raise ValueError(f"{where}: {name} is {t.dtype}, not float32")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{where}: {name} is {tuple(t.shape)}, not {tuple(shape)}")
    if t.device != dev:
        raise ValueError(f"{where}: {name} is on {t.device}, not on {dev}")
    if not t.is_contiguous() or t.data_ptr() % 16 != 0:
        raise ValueError(f"{where}: {name} is not contiguous from a 16-byte boundary")


def _group_slots(opt, p):
    return [(g, i) for g in opt.param_groups for i, q in enumerate(g["params"]) if q is p]


def held_arrays(params: GaussianParams, opt, where: str):
    """The five raw arrays of `params` and the moments `opt` holds of them, refused (ValueError, `where` in front) unless the
    kernels can take them: see densify_and_prune. -> (old {name: parameter}, n, device, held {name: (exp_avg, exp_avg_sq)})"""
    old = {k: getattr(params, k) for k in RAW}
    n, dev = int(old["xyz"].shape[0]), old["xyz"].device
    if not old["xyz"].is_cuda:
        raise ValueError(f"{where}: the parameters are on {dev}, not on a GPU")
    held = {}
    for k in RAW:
        shape = (n,) if k == "opacity_logit" else (n, ROW_FLOATS[k])
        _refuse(old[k], k, shape, dev, where)
        if opt is not None:
            if not _group_slots(opt, old[k]):
                raise ValueError(f"{where}: the optimiser does not hold {k}")
            state = opt.state[old[k]] if old[k] in opt.state else {}
            have = [m for m in MOMENTS if m in state]
            if len(have) == 1:
                raise ValueError(f"{where}: the optimiser's state of {k} has {have[0]} alone")
            for m in have:
                _refuse(state[m], f"state {m} of {k}", shape, dev, where)
            if have:
                held[k] = (state["exp_avg"], state["exp_avg_sq"])
    return old, n, dev, held


def gather_rows(old, held, n: int, counts, src_of: torch.Tensor, noise, log_shrink: float, dev):
    """gsr_densify_apply into fresh arrays of counts[3] rows. -> (fresh {name: tensor}, fresh_moments {name: (m, v)})"""
    kept, clones, splits, total = counts
    fresh = {k: torch.empty((total,) + tuple(old[k].shape[1:]), dtype=torch.float32, device=dev) for k in RAW}
    fresh_moments = {k: tuple(torch.empty_like(fresh[k]) for _ in MOMENTS) for k in held}
    if total > 0:
        a = _capi.DensifyApplyArgs()
        a.struct_size, a.log_shrink, a.n_src = C.sizeof(_capi.DensifyApplyArgs), log_shrink, n
        a.counts[:] = [kept, clones, splits, total]
        a.src_of, a.noise, a.stream = src_of.data_ptr(), noise.data_ptr() if splits else None, _capi.stream(dev)
        for k in RAW:
            arr = getattr(a, k)
            arr.src, arr.dst = old[k].data_ptr(), fresh[k].data_ptr()
            if k in held:
                arr.src_exp_avg, arr.src_exp_avg_sq = (t.data_ptr() for t in held[k])
                arr.dst_exp_avg, arr.dst_exp_avg_sq = (t.data_ptr() for t in fresh_moments[k])
        _capi.call("gsr_densify_apply", C.byref(a), device=dev)
    return fresh, fresh_moments


def replace_parameters(params: GaussianParams, opt, old, held, fresh, fresh_moments) -> None:
    """The five nn.Parameters of `params` replaced by new ones over `fresh`; opt's param_groups entries swapped in place and
    its state re-keyed ("step" kept, the moments — only where there were any — replaced by fresh_moments)."""
    for k in RAW:
        p = torch.nn.Parameter(fresh[k], requires_grad=old[k].requires_grad)
        setattr(params, k, p)
        if opt is None:
            continue
        for group, i in _group_slots(opt, old[k]):
            group["params"][i] = p
        if old[k] in opt.state:
            state = opt.state.pop(old[k])
            if k in held:
                state["exp_avg"], state["exp_avg_sq"] = fresh_moments[k]
            opt.state[p] = state


def densify_and_prune(params: GaussianParams, opt, stats: DensityStats, *, max_grad: float = 0.0002, min_opacity: float = 0.005,
                      extent: float, max_screen_size: "int | None" = None, percent_dense: float = 0.01, generator=None):
    """Upstream's densify_and_prune in three HIP calls. With g = grad_accum / denom (0 where never seen) and m the largest
    log-scale of a Gaussian: g >= max_grad clones it where exp(m) <= percent_dense * extent and otherwise splits it into two
    children drawn from it (scales divided by 1.6, moved by its own covariance times `torch.randn((S, 2, 3),
    generator=generator)`); then everything with opacity < min_opacity goes, and with max_screen_size also what was seen
    larger than that many pixels or is larger than 0.1 * extent in the world (a clone or child is tested with its parent's
    radius). Rows of the result: the kept Gaussians in their order, the clones, child 0 of every split, child 1 of each.

    The five nn.Parameters of `params` are replaced by new ones (gradients None). opt (a GaussianAdam or torch.optim.Adam
    that holds all five, or None): its param_groups entries are swapped in place and its state is re-keyed: "step" is kept,
    the moments — only where there were any — follow their rows, zeros for clones and children. `stats` restarts from zeros
    at the new row count. One synchronisation (the counts). Returns (src_of i32[N_new]: the old row of every new row;
    (K, C, S, N_new): kept, clones, splits that survived, the new row count).

    With statistics accumulated by DensityStats.update(absgrad=True) g is the mean of AbsGS's absolute score, which is never
    below the signed norm and usually several times it: max_grad is then on another scale. gsplat suggests 0.0008 where 0.0002
    serves the signed norm; that figure is gsplat's and has not been measured here.

    Raises ValueError before anything is launched or replaced: a parameter of `params` that `opt` does not hold; parameters
    or moments that are not float32, of the wrong shape, on another device, not contiguous from a 16-byte boundary; one
    moment without the other; `stats` of another length or device."""
    old, n, dev, held = held_arrays(params, opt, "densify_and_prune")
    if not isinstance(stats, DensityStats) or stats.num_gaussians != n or stats.device != dev:
        raise ValueError(f"densify_and_prune: the statistics are not those of {n} Gaussians on {dev}")
    if not (0.0 < min_opacity < 1.0 and extent > 0.0 and percent_dense > 0.0):
        raise ValueError("densify_and_prune: min_opacity must lie in (0, 1), extent and percent_dense above 0")
    scalars = plan_scalars(float(max_grad), float(min_opacity), float(extent), float(percent_dense))
    max_screen = int(max_screen_size) if max_screen_size is not None else 0
    # ---- nothing is refused from here on ----
    new_i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    if n == 0:
        return new_i32(0), (0, 0, 0, 0)
    stream = _capi.stream(dev)
    temp = torch.empty(int(_capi.lib().gsr_densify_plan_temp_bytes(n)), dtype=torch.uint8, device=dev)
    src_of, counts = new_i32(3 * n), new_i32(4)
    _capi.call("gsr_densify_plan", n, old["opacity_logit"].data_ptr(), old["log_scale"].data_ptr(), stats.grad_accum.data_ptr(),
               stats.denom.data_ptr(), stats.max_radii.data_ptr(), *scalars, max_screen, temp.data_ptr(), src_of.data_ptr(),
               counts.data_ptr(), stream, device=dev)
    kept, clones, splits, total = (int(c) for c in counts.tolist())                    # (the one synchronisation)
    noise_dev = generator.device if generator is not None else dev
    noise = torch.randn((splits, 2, 3), generator=generator, dtype=torch.float32, device=noise_dev).to(dev).contiguous()
    fresh, fresh_moments = gather_rows(old, held, n, (kept, clones, splits, total), src_of, noise, scalars[4], dev)
    replace_parameters(params, opt, old, held, fresh, fresh_moments)
    stats.reset(total)
    return src_of[:total], (kept, clones, splits, total)


def reset_opacity(params: GaussianParams, opt=None, ceiling: float = 0.01) -> None:
    """Upstream's reset_opacity: no opacity above `ceiling` afterwards (opacity_logit clamped to logit(ceiling), in place),
    and the optimiser's two moments of opacity_logit zeroed, where it has any. The writes bump the tensors' version
    counters, as GaussianAdam.step's do."""
    if not 0.0 < ceiling < 1.0:
        raise ValueError(f"reset_opacity: a ceiling of {ceiling}")
    p = params.opacity_logit
    with torch.no_grad():
        p.clamp_(max=math.log(ceiling / (1.0 - ceiling)))
        if opt is not None and p in opt.state:
            for m in MOMENTS:
                if m in opt.state[p]:
                    opt.state[p][m].zero_()
