"""Per-Gaussian contribution statistics of the training views, exact, and the row removal that goes with them
(gsr_contribution, csrc/contrib.hip; include/gsrast_amd_contrib.h states the quantity operation by operation).

    stats = ContributionStats(params.num_gaussians, dev)
    with torch.no_grad():
        for cam in training_views:
            render(params, rast, cam)
            stats.update(rast)                                   # one launch; sums add up, maxima take the larger
    prune_rows(params, opt, stats.weight_max >= 0.01)            # the score is the trainer's expression

The blending weight alpha_i T_i of a Gaussian at a pixel is taken in fixed point, q = floor(alpha T 2^32): sums of integers do
not depend on the order they are added in, so every statistic is bit for bit reproducible over runs, streams and view orders.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi
from . import densify
from .autograd import GaussianParams

WHAT = ("weight_sum", "weight_max", "pixels", "dominant")
_DTYPE = {"weight_sum": torch.int64, "weight_max": torch.int32, "pixels": torch.int64, "dominant": torch.int64}
_SCALE = 2.0 ** -32


class ContributionStats:
    """Four statistics per Gaussian over the frames since reset(), any subset of them (`what`):
    weight_sum — the sum over pixels of its blending weight; weight_max — its largest blending weight at any pixel;
    pixels — how many pixels blended it; dominant — at how many pixels its weight was the largest (a tie: the front-most)."""

    def __init__(self, n: int, device, what=WHAT):
        what = tuple(what)
        if not what or any(w not in WHAT for w in what) or len(set(what)) != len(what):
            raise ValueError(f"ContributionStats: what={what!r}; a non-empty choice of {WHAT}")
        self.device = torch.device(device)
        self.what = what
        self.reset(n)

    def reset(self, n: "int | None" = None) -> None:
        """Zeros, at a new row count if one is given."""
        n = self.num_gaussians if n is None else int(n)
        # (u64 / u32 on the device; torch sees them as int64 / int32: no count here reaches the sign bit, weight_max is read unsigned)
        self.raw = {w: torch.zeros(n, dtype=_DTYPE[w], device=self.device) for w in self.what}
        self.frames = 0

    @property
    def num_gaussians(self) -> int:
        return int(next(iter(self.raw.values())).shape[0])

    def _get(self, name: str) -> torch.Tensor:
        if name not in self.raw:
            raise AttributeError(f"ContributionStats: {name} is not collected (what={self.what})")
        return self.raw[name]

    @property
    def weight_sum(self) -> torch.Tensor:
        """float64[N]: the summed blending weight (the integer sum times 2^-32: exact up to 2^53 / 2^32 pixels' worth)."""
        return self._get("weight_sum").to(torch.float64) * _SCALE

    @property
    def weight_max(self) -> torch.Tensor:
        """float32[N]: the largest blending weight at any pixel of any frame."""
        return ((self._get("weight_max").to(torch.int64) & 0xFFFFFFFF).to(torch.float64) * _SCALE).to(torch.float32)

    @property
    def pixels(self) -> torch.Tensor:
        return self._get("pixels")

    @property
    def dominant(self) -> torch.Tensor:
        return self._get("dominant")

    def update(self, rast, *, semantics: str = "gscuda", receipt: "_capi.ForwardReceipt | None" = None) -> None:
        """Adds the frame of `rast`'s last draw() / render() (or of `receipt`, while the chunks still hold that call): one
        launch on the current stream, no synchronisation. It must run before that rasterizer draws again; it writes nothing
        a later backward() reads, so it may sit between render() and loss.backward(). ValueError before anything is
        launched: no frame yet, a draw(sorted_lists=False), another N or another device than the statistics'."""
        if semantics not in ("gscuda", "inria"):
            raise ValueError(f"ContributionStats.update: semantics={semantics!r}")
        rcpt = receipt if receipt is not None else rast.last_receipt
        if rcpt is None:
            raise ValueError("ContributionStats.update: the rasterizer has drawn no frame")
        n = self.num_gaussians
        if rast.device != self.device:
            raise ValueError(f"ContributionStats.update: the statistics are on {self.device}, the rasterizer on {rast.device}")
        if rast.num_gaussians != n or int(rcpt.num_gaussians) != n:
            raise ValueError(f"ContributionStats.update: the statistics have {n} rows, the frame has "
                             f"{int(rcpt.num_gaussians)} Gaussians")
        if int(rcpt.plan_used) & _capi.GSR_PLAN_LISTS_SKIPPED:
            raise ValueError("ContributionStats.update: that draw() skipped its sorted lists (sorted_lists=False)")
        a = contribution_args(rast, rcpt, semantics, {w: t.data_ptr() for w, t in self.raw.items()})
        _capi.call("gsr_contribution", C.byref(a), device=self.device)
        self.frames += 1


def contribution_args(rast, rcpt: "_capi.ForwardReceipt", semantics: str, outputs: dict) -> "_capi.ContributionArgs":
    """gsr_contribution_args for the forward call of `rcpt` on `rast`, on torch's current stream: that call's chunks mapped
    as backward() maps them. outputs: {name of WHAT: device address}; the others stay NULL."""
    a = _capi.ContributionArgs()
    a.struct_size = C.sizeof(_capi.ContributionArgs)
    a.flags = _capi.GSR_FLAG_SEMANTICS_INRIA if semantics == "inria" else 0
    a.num_gaussians, a.width, a.height = rast.num_gaussians, rast.width, rast.height
    rast._map_frame(a, int(rcpt.num_rendered))
    a.receipt = rcpt
    for w, ptr in outputs.items():
        assert w in WHAT, w
        setattr(a, w, ptr)
    a.stream = _capi.stream(rast.device)
    return a


def prune_rows(params: GaussianParams, opt, keep: torch.Tensor) -> torch.Tensor:
    """Removes the rows where `keep` is False from the five parameters of `params` and from the moments `opt` holds of them
    (a GaussianAdam or torch.optim.Adam that holds all five, or None) through gsr_densify_apply: the kept rows in ascending
    order, "step" kept, no new rows; the parameters are replaced as densify_and_prune replaces them. Returns src_of
    (i32[N_new]: the old row of every new row). ValueError before anything is replaced: `keep` not a bool tensor of N
    elements on the parameters' device, and everything densify_and_prune refuses of `params` and `opt`. All True: nothing
    is launched or replaced. One synchronisation (the number of kept rows)."""
    old, n, dev, held = densify.held_arrays(params, opt, "prune_rows")
    if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool:
        raise ValueError(f"prune_rows: keep is {getattr(keep, 'dtype', type(keep))}, not a bool tensor")
    if tuple(keep.shape) != (n,):
        raise ValueError(f"prune_rows: keep is {tuple(keep.shape)}, not ({n},)")
    if keep.device != dev:
        raise ValueError(f"prune_rows: keep is on {keep.device}, not on {dev}")
    src_of = torch.nonzero(keep).reshape(-1).to(torch.int32)          # (ascending; the synchronisation)
    kept = int(src_of.shape[0])
    if kept == n:
        return src_of
    fresh, fresh_moments = densify.gather_rows(old, held, n, (kept, 0, 0, kept), src_of, None, 0.0, dev)
    densify.replace_parameters(params, opt, old, held, fresh, fresh_moments)
    return src_of
