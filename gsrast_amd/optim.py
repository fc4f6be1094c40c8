"""GaussianAdam: torch.optim.Adam's update as one HIP launch (gsr_adam_step, csrc/adam.hip) that skips the Gaussians a
frame culled.

    slot = RadiiSlot()
    color, _, _ = render(params, rast, cam, radii_slot=slot)
    loss(color).backward()
    opt.step(slot.radii)                 # i32[N]: a Gaussian with radii[i] <= 0 keeps its parameters and both moments

`step()` without an argument is the dense update: torch.optim.Adam's formula in the operation order include/gsrast_amd.h
states. With a visibility array it is a sparse Adam in the sense of torch.optim.SparseAdam: the moments of a Gaussian the
frame did not see stand still (a dense Adam decays them and keeps moving the Gaussian by its stale momentum), and the bias
correction is by the optimiser's global step count, not by how often a Gaussian was seen.

The kernel writes through raw pointers, in place, on the current stream, and does not synchronise.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _capi


def adam_scalars(lr: float, beta1: float, beta2: float, eps: float, step: int):
    """The six floats gsr_adam_step takes for Adam's step `step` (>= 1), computed in double; ctypes rounds each to float
    once. (step_size, rs, b1c, b2, b2c, eps)"""
    return (lr / (1.0 - beta1 ** step), math.sqrt(1.0 - beta2 ** step), 1.0 - beta1, beta2, 1.0 - beta2, eps)


def _refuse(t: torch.Tensor, name: str) -> None:
    """What the kernel cannot take of a tensor's layout: an in-place update cannot clone its way out of it."""
    if t.dtype != torch.float32:
        raise ValueError(f"GaussianAdam: {name} is {t.dtype}, not float32")
    if t.layout != torch.strided:
        raise ValueError(f"GaussianAdam: {name} is sparse")
    if not t.is_contiguous():
        raise ValueError(f"GaussianAdam: {name} is not contiguous")
    if t.data_ptr() % 16 != 0:
        raise ValueError(f"GaussianAdam: {name} does not start on a 16-byte boundary")


class GaussianAdam(torch.optim.Optimizer):
    """Adam over float32 GPU parameters whose first dimension is the Gaussian: torch.optim.Adam's arguments and defaults
    (no weight decay, amsgrad or maximize), its param_groups (a learning rate per group, read at every step) and its state
    keys "step", "exp_avg", "exp_avg_sq" — code that prunes or densifies by editing an Adam's state applies unchanged
    (gsrast_amd.densify.densify_and_prune does it in one HIP launch)."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8):
        if not lr >= 0.0:
            raise ValueError(f"invalid learning rate: {lr}")
        if not eps >= 0.0:
            raise ValueError(f"invalid eps: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas: {betas}")
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps))

    @torch.no_grad()
    def step(self, visibility: "torch.Tensor | None" = None) -> None:
        """One update of every parameter that has a gradient; one without is skipped entirely (state and step count too).

        visibility: None — every element is updated, whatever the parameters' shapes. i32[N] (a frame's radii, or the
        torch.maximum of several frames') or bool[N] — row i of every parameter is updated iff visibility[i] > 0; every
        parameter updated in this call must then have shape[0] == N. The step count advances for every parameter with a
        gradient, visible rows or not. Raises ValueError before anything is launched or changed for a parameter, gradient or
        state tensor the kernel cannot take: not float32, not contiguous, not on a GPU, not starting on a 16-byte boundary, a
        sparse gradient or one of another shape."""
        todo = []                                           # (parameter, its group, its state)
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                _refuse(p, "a parameter")
                if p.grad.shape != p.shape:
                    raise ValueError(f"GaussianAdam: a gradient is {tuple(p.grad.shape)}, its parameter {tuple(p.shape)}")
                _refuse(p.grad, "a gradient")
                state = self.state[p]
                held = [(k, state[k]) for k in ("exp_avg", "exp_avg_sq") if k in state]
                for k, t in held:
                    if t.shape != p.shape:
                        raise ValueError(f"GaussianAdam: state {k} is {tuple(t.shape)}, its parameter {tuple(p.shape)}")
                    _refuse(t, f"state {k}")
                if not p.is_cuda:
                    raise ValueError(f"GaussianAdam: a parameter is on {p.device}, not on a GPU")
                for k, t in [("gradient", p.grad)] + held:
                    if t.device != p.device:
                        raise ValueError(f"GaussianAdam: a parameter is on {p.device}, its {k} on {t.device}")
                todo.append((p, group, state))
        if not todo:
            return
        if visibility is not None:
            dev = todo[0][0].device
            if visibility.dtype not in (torch.int32, torch.bool) or visibility.dim() != 1:
                raise ValueError(f"GaussianAdam: visibility is {visibility.dtype} {tuple(visibility.shape)}, not i32[N] or bool[N]")
            n = int(visibility.shape[0])
            for p, _, _ in todo:
                if p.dim() == 0 or int(p.shape[0]) != n or p.device != dev:
                    raise ValueError(f"GaussianAdam: visibility has {n} rows on {visibility.device}, a parameter is "
                                     f"{tuple(p.shape)} on {p.device}")
            if visibility.device != dev:
                raise ValueError(f"GaussianAdam: visibility is on {visibility.device}, the parameters on {dev}")
            visibility = visibility.to(torch.int32).contiguous()
        # ---- nothing is refused from here on (a new moment tensor is an allocation of its own: contiguous and aligned) ----
        calls = {}                                          # (device, rows) -> [(p, g, m, v, row_floats, scalars)]
        for p, group, state in todo:
            if "exp_avg" not in state:
                state["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            if "exp_avg_sq" not in state:
                state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            t = int(state.get("step", 0)) + 1               # (a tensor in a torch.optim.Adam state dict)
            state["step"] = t
            if p.numel() == 0:
                continue
            rows = int(p.shape[0]) if p.dim() else 1        # (a row is a Gaussian; dense, any split into rows gives the same bits)
            beta1, beta2 = group["betas"]
            scalars = adam_scalars(float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), t)
            calls.setdefault((p.device, rows), []).append((p, p.grad, state["exp_avg"], state["exp_avg_sq"], p.numel() // rows, scalars))
        for (dev, rows), tensors in calls.items():
            for at in range(0, len(tensors), _capi.GSR_ADAM_MAX_TENSORS):
                part = tensors[at:at + _capi.GSR_ADAM_MAX_TENSORS]
                a = _capi.AdamArgs()
                a.struct_size, a.num_tensors, a.num_rows = C.sizeof(_capi.AdamArgs), len(part), rows
                a.visible = visibility.data_ptr() if visibility is not None else None
                a.stream = _capi.stream(dev)
                for slot, (p, g, m, v, row_floats, scalars) in zip(a.tensors, part):
                    slot.param, slot.grad, slot.exp_avg, slot.exp_avg_sq = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
                    slot.row_floats = row_floats
                    slot.step_size, slot.rs, slot.b1c, slot.b2, slot.b2c, slot.eps = scalars
                _capi.call("gsr_adam_step", C.byref(a), device=dev)
            for p, _, m, v, _, _ in tensors:
                # the kernel wrote through raw pointers: autograd's saved-tensor check and whatever keys on ._version
                # (SplatRasterizer.precomputed_colors) must see the write
                for t in (p, m, v):
                    torch.autograd.graph.increment_version(t)
