"""CPU: the photometric loss as include/gsrast_amd.h states it (tests/ssim_ref.py, its numpy restatement) — in float64 against
torch's float64 autograd of the conv2d composition every trainer writes, in float32 against the same reference within the
float32 restatement's own error, its exact cases (black images, equal images, the upstream scalar), the header's window, and
every refusal of the C entry points (null or made-up pointers: no GPU is touched)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import ssim_ref as R
from helpers import ROOT

from gsrast_amd import _capi

SHAPES = [(3, 45, 70), (3, 7, 5), (3, 33, 64), (1, 1, 1)]
SEED = 11
LAMBDA = 0.2


@functools.lru_cache(maxsize=None)
def _reference(shape):
    """torch, float64, on the float32 inputs of ssim_ref.images(shape, SEED): five depthwise 11 x 11 conv2d calls, the SSIM
    map, the loss, and autograd's gradient. -> dict of numpy arrays and floats (read only)."""
    import torch
    import torch.nn.functional as F
    xn, yn = R.images(shape, SEED)
    x = torch.tensor(xn, dtype=torch.float64, requires_grad=True)
    y = torch.tensor(yn, dtype=torch.float64)
    g = torch.tensor(R.window(np.float64))
    channels = shape[0]
    w2 = (g[:, None] * g[None, :])[None, None].expand(channels, 1, R.TAPS, R.TAPS).contiguous()
    conv = lambda a: F.conv2d(a[None], w2, padding=R.RADIUS, groups=channels)[0]
    mu1, mu2 = conv(x), conv(y)
    s11, s22, s12 = conv(x * x) - mu1 * mu1, conv(y * y) - mu2 * mu2, conv(x * y) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    l1, ssim = (x - y).abs().mean(), m.mean()
    loss = (1 - LAMBDA) * l1 + LAMBDA * (1 - ssim)
    loss.backward()
    out = {"m": m.detach().numpy(), "grad": x.grad.numpy(), "terms": (loss.item(), l1.item(), ssim.item())}
    for a in (out["m"], out["grad"]):
        a.setflags(write=False)
    return out


# ---- 1. the formulas -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_restatement_is_torchs_autograd_of_the_conv2d_composition(shape):
    ref = _reference(shape)
    x, y = R.images(shape, SEED)
    m = R.maps(x, y, np.float64)["m"]
    grad = R.gradient(x, y, LAMBDA, 1.0, np.float64)
    terms = R.terms(x, y, LAMBDA, np.float64)
    scale = np.abs(ref["grad"]).max()
    e_map, e_grad = np.abs(m - ref["m"]).max(), np.abs(grad - ref["grad"]).max() / scale
    e_terms = max(abs(a - b) for a, b in zip(terms, ref["terms"]))
    print(f"[photo loss f64] {shape}: map {e_map:.2e}, gradient {e_grad:.2e} of max|grad|, terms {e_terms:.2e}")
    assert scale > 0
    assert e_map <= 1e-12 and e_grad <= 1e-12 and e_terms <= 1e-12


# ---- 2. float32 ------------------------------------------------------------------------------------------------------------
# Each bound is 4 x the largest error these inputs show over SHAPES (the cancellation in conv(x*x) - mu1*mu1 moves the error
# by tens of per cent from seed to seed: 1.9 .. 3.5e-6 for the map, 2.7 .. 5.3e-7 for the gradient over six seeds).
MAP_BOUND = 4 * 2.45e-6           # measured 2.442e-06, on (3,45,70)
GRAD_BOUND = 4 * 3.30e-7          # measured 3.292e-07 of max|grad|, on (3,45,70)
TERM_BOUNDS = (4 * 7.6e-9, 4 * 7.8e-12, 4 * 3.8e-8)      # loss 7.52e-09, l1 7.76e-12, ssim 3.76e-08, all on (3,7,5)


@pytest.mark.parametrize("shape", SHAPES)
def test_float32_restatement_is_within_its_own_rounding_of_the_float64_reference(shape):
    ref = _reference(shape)
    x, y = R.images(shape, SEED)
    q = R.maps(x, y, np.float32)
    grad = R.gradient(x, y, LAMBDA, 1.0, np.float32)
    assert q["m"].dtype == np.float32 and grad.dtype == np.float32
    terms = R.terms(x, y, LAMBDA, np.float32)
    e_map = np.abs(q["m"].astype(np.float64) - ref["m"]).max()
    e_grad = np.abs(grad.astype(np.float64) - ref["grad"]).max() / np.abs(ref["grad"]).max()
    e_terms = [abs(a - b) for a, b in zip(terms, ref["terms"])]
    print(f"[photo loss f32] {shape}: map {e_map:.3e}, gradient {e_grad:.3e} of max|grad|, terms " + " ".join(f"{e:.2e}" for e in e_terms))
    assert e_map <= MAP_BOUND and e_grad <= GRAD_BOUND
    assert all(e <= b for e, b in zip(e_terms, TERM_BOUNDS))


# ---- 3. the exact cases ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_black_images_have_ssim_one_and_no_gradient(dtype):
    z = np.zeros((3, 13, 17), np.float32)
    assert (R.maps(z, z, dtype)["m"] == 1).all()
    for lam in (0.0, 0.2, 1.0):
        assert (R.gradient(z, z, lam, 1.0, dtype) == 0).all()
        loss, l1, ssim = R.terms(z, z, lam, dtype)
        assert (loss, l1, ssim) == (0.0, 0.0, 1.0)


def test_equal_images_have_no_l1_gradient_and_the_upstream_scalar_scales():
    x, y = R.images((3, 33, 64), SEED)
    assert (R.gradient(x, x, 0.0, 1.0) == 0).all()                       # lambda = 0: the L1 term alone, sgn == 0 everywhere
    h, w = 33 // 4, 64 // 4
    assert (x[:, 33 - h:, 64 - w:] == y[:, 33 - h:, 64 - w:]).all()        # (the block of ssim_ref.images where image == target)
    block = R.gradient(x, y, 0.0, 1.0)[:, 33 - h:, 64 - w:]
    assert (block == 0).all()
    one, part = R.gradient(x, y, LAMBDA, 1.0), R.gradient(x, y, LAMBDA, 0.37)
    assert (one != 0).any()
    assert (part.view(np.uint32) == (np.float32(0.37) * one).view(np.uint32)).all()


def test_the_header_spells_out_the_window():
    text = open(os.path.join(ROOT, "include", "gsrast_amd.h")).read()
    body = re.search(r"#define GSR_PHOTO_LOSS_WINDOW \{(.*?)\}", text, flags=re.S).group(1)
    floats = np.array([np.float32(t.strip().rstrip("f")) for t in body.replace("\\", " ").split(",")], np.float32)
    assert floats.shape == (R.TAPS,)
    assert (floats.view(np.uint32) == R.window(np.float32).view(np.uint32)).all()


# ---- 4. what the C entry points refuse -------------------------------------------------------------------------------------
def _valid_args():
    """Arguments both calls would take, over made-up (aligned, non-null) addresses: every test below breaks one thing, so
    that the call returns before it launches anything."""
    a = _capi.PhotoLossArgs()
    a.struct_size = C.sizeof(_capi.PhotoLossArgs)
    a.channels, a.width, a.height, a.lambda_dssim = 3, 64, 32, 0.2
    a.image, a.target, a.scratch, a.out, a.dL_dloss, a.dL_dimage = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.want_backward = 1
    return a


BROKEN = ([("struct_size", C.sizeof(_capi.PhotoLossArgs) - 4), ("struct_size", 0), ("channels", 0), ("width", 0), ("height", -1),
           ("lambda_dssim", -0.01), ("lambda_dssim", 1.01), ("lambda_dssim", float("nan"))]
          + [(k, None) for k in ("image", "target", "scratch")] + [(k, 0x10004) for k in ("image", "target", "scratch")])


@pytest.mark.parametrize("call,own", [("gsr_photo_loss_forward", [("out", None), ("out", 0x40002)]),
                                      ("gsr_photo_loss_backward", [("dL_dloss", None), ("dL_dloss", 0x50001), ("dL_dimage", None),
                                                                   ("dL_dimage", 0x60008)])])
def test_the_calls_refuse_before_they_launch(call, own):
    L = _capi.lib()
    fn = getattr(L, call)
    assert fn(None) == _capi.GSR_ERR_INVALID_ARG
    for field, value in BROKEN + own:
        a = _valid_args()
        setattr(a, field, value)
        assert fn(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG, (call, field, value)
        assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG


@pytest.mark.parametrize("call", ["gsr_photo_loss_forward", "gsr_photo_loss_backward"])
def test_an_image_of_more_floats_than_an_int_counts_is_too_large(call):
    L = _capi.lib()
    for c, w, h in ((3, 32768, 32768), (70000, 8, 8), (1, 8, 65535 * 16 + 1)):
        a = _valid_args()
        a.channels, a.width, a.height = c, w, h
        assert getattr(L, call)(C.byref(a)) == _capi.GSR_ERR_TOO_LARGE, (c, w, h)
        assert L.gsr_photo_loss_scratch_bytes(c, w, h) == 0


def test_scratch_bytes_hold_the_partial_sums_and_three_maps():
    L = _capi.lib()
    for c, w, h in ((3, 1920, 1080), (3, 5, 7), (1, 1, 1), (3, 197, 131)):
        n = L.gsr_photo_loss_scratch_bytes(c, w, h)
        assert n >= 12 * c * w * h + 16                                  # (at least one workgroup's pair of doubles)
    assert L.gsr_photo_loss_scratch_bytes(0, 5, 7) == 0 and L.gsr_photo_loss_scratch_bytes(3, -1, 7) == 0


def test_the_ctypes_struct_has_the_headers_layout(tmp_path):
    import subprocess
    fields = [f for f, _ in _capi.PhotoLossArgs._fields_]
    lines = ['printf("size %zu\\n", sizeof(gsr_photo_loss_args));']
    lines += [f'printf("{f} %zu\\n", offsetof(gsr_photo_loss_args, {f}));' for f in fields]
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + "".join(lines) + "return 0;}")
    exe = tmp_path / "probe"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["size"]) == C.sizeof(_capi.PhotoLossArgs)
    for f in fields:
        assert int(got[f]) == getattr(_capi.PhotoLossArgs, f).offset, f
