"""photometric_loss: the 3DGS training loss (1 - lambda) * L1 + lambda * (1 - SSIM), value and gradient as fused HIP kernels
(gsr_photo_loss_forward / _backward, csrc/photo_loss.hip; include/gsrast_amd.h states the arithmetic).

    color, _, _ = render(params, rast, cam, radii_slot=slot)
    loss = photometric_loss(color, target)          # lambda_dssim = 0.2, the 11 x 11 window with sigma 1.5, zero padded
    loss.backward()
    opt.step(slot.radii)

Ownership (the rule of autograd.py): the three loss terms, the scratch the forward hands to the backward and the gradient
are new tensors of the call that makes them, written by no later call; two graphs alive at once share nothing. The upstream
gradient reaches the kernel as a device pointer: nothing here synchronises or reads a value back to the host.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from . import _capi

F32 = torch.float32


def _args(image, target, lam, scratch):
    a = _capi.PhotoLossArgs()
    a.struct_size = C.sizeof(_capi.PhotoLossArgs)
    a.channels, a.height, a.width = (int(s) for s in image.shape)
    a.lambda_dssim = lam
    a.image, a.target, a.scratch = image.data_ptr(), target.data_ptr(), scratch.data_ptr()
    a.stream = _capi.stream(image.device)
    return a


class _PhotoLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, image, target, lam):
        dev = image.device
        image, target = _capi.aligned16(image.detach()), _capi.aligned16(target.detach())
        want = bool(ctx.needs_input_grad[0])
        c, h, w = (int(s) for s in image.shape)
        scratch = torch.empty(_capi.lib().gsr_photo_loss_scratch_bytes(c, w, h), dtype=torch.uint8, device=dev)
        out = torch.empty(3, dtype=F32, device=dev)
        a = _args(image, target, lam, scratch)
        a.out, a.want_backward = out.data_ptr(), int(want)
        _capi.call("gsr_photo_loss_forward", C.byref(a), device=dev)
        if want:
            ctx.save_for_backward(image, target)                # (a write to either before backward() is reported)
            ctx.scratch, ctx.out, ctx.lam = scratch, out, lam
        loss, l1, ssim = out[0], out[1], out[2]
        ctx.mark_non_differentiable(l1, ssim)
        return loss, l1, ssim

    @staticmethod
    @once_differentiable
    def backward(ctx, up, _l1, _ssim):
        if up is None or not ctx.needs_input_grad[0]:
            return None, None, None
        image, target = ctx.saved_tensors
        dev = image.device
        up = up.to(device=dev, dtype=F32).contiguous()          # (a 0-dim float32 tensor of this device as it comes: nothing is copied)
        grad = torch.empty_like(image)
        a = _args(image, target, ctx.lam, ctx.scratch)
        a.dL_dloss, a.dL_dimage = up.data_ptr(), grad.data_ptr()
        _capi.call("gsr_photo_loss_backward", C.byref(a), device=dev)
        return grad, None, None


def photometric_loss(image: torch.Tensor, target: torch.Tensor, lambda_dssim: float = 0.2, return_terms: bool = False):
    """(1 - lambda_dssim) * mean|image - target| + lambda_dssim * (1 - SSIM(image, target)): a 0-dim float32 tensor on the
    images' device, differentiable with respect to `image` (not `target`). image, target: float32 [C,H,W] on one GPU, of one
    shape; a non-contiguous view, or one that does not start on a 16-byte boundary, is copied. return_terms: (loss, l1, ssim),
    the last two detached 0-dim tensors. When `image` requires no gradient the forward writes nothing for a backward.
    Raises ValueError before anything is launched for a tensor that is not float32, not [C,H,W] or empty, not on a GPU, on
    another device or of another shape than its partner, and for lambda_dssim outside [0, 1]."""
    for name, t in (("image", image), ("target", target)):
        if not isinstance(t, torch.Tensor) or t.dtype != F32:
            raise ValueError(f"photometric_loss: {name} is {getattr(t, 'dtype', type(t))}, not float32")
        if t.dim() != 3 or t.numel() == 0:
            raise ValueError(f"photometric_loss: {name} is {tuple(t.shape)}, not [C,H,W]")
        if not t.is_cuda:
            raise ValueError(f"photometric_loss: {name} is on {t.device}, not on a GPU")
    if image.device != target.device:
        raise ValueError(f"photometric_loss: image is on {image.device}, target on {target.device}")
    if image.shape != target.shape:
        raise ValueError(f"photometric_loss: image is {tuple(image.shape)}, target {tuple(target.shape)}")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"photometric_loss: lambda_dssim is {lambda_dssim}, outside [0, 1]")
    loss, l1, ssim = _PhotoLoss.apply(image, target, lam)
    return (loss, l1, ssim) if return_terms else loss
