"""What the training loss costs at 3 x 1080 x 1920 on one GPU: gsrast_amd.loss.photometric_loss (gsr_photo_loss_forward /
_backward) — the two C calls alone, both, and through autograd — against the plain float32 torch composition every trainer
writes (five depthwise conv2d calls with the 11 x 11 outer-product window, groups=3, padding=5, and the elementwise SSIM
formula; autograd's backward); then the whole training step on the bench scene, render() + loss + backward() +
GaussianAdam.step(radii), with the L1 loss of the earlier cost tables, the torch composition and the fused loss. The image is
the bench frame, the target the same frame with noise. Bytes: what the algorithm needs (image and target read, gradient
written: 12 per image float) and what these kernels move (44: the three derivative maps make a round trip and the backward
reads image and target again). Medians of device-event times, every configuration after its own warm-up, configurations
interleaved round by round.
Usage: python scripts/photo_loss_cost.py [--reps N] [--splats N] [--out FILE]   (the table of profiles/photo_loss_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
FLOATS = 3 * H * W
NEEDED, MOVED = 12 * FLOATS, 44 * FLOATS
LAMBDA = 0.2


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 30)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)
HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s (spec)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def interleaved(fns):
    """name -> median ms: three warm-up rounds, then REPS rounds, each running every configuration once."""
    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(REPS):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ms.items()}


def share(ms, nbytes):
    return f"{nbytes / (ms * 1e-3) / 1e12:.2f} TB/s = {100 * nbytes / (ms * 1e-3) / HBM_PEAK:.1f} %"


def torch_ssim_loss(window2d):
    def loss(image, target):
        conv = lambda a: F.conv2d(a[None], window2d, padding=5, groups=3)[0]
        mu1, mu2 = conv(image), conv(target)
        s11 = conv(image * image) - mu1 * mu1
        s22 = conv(target * target) - mu2 * mu2
        s12 = conv(image * target) - mu1 * mu2
        C1, C2 = 0.01 ** 2, 0.03 ** 2
        m = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
        return (1.0 - LAMBDA) * (image - target).abs().mean() + LAMBDA * (1.0 - m.mean())
    return loss


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    make = lambda: GaussianParams.from_raw(*raw, device=dev)
    out = [f"photometric loss cost, 3 x {H} x {W}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds",
           f"bench frame ({label})"]

    # ---- the frame and its target ----
    with torch.no_grad():
        frame = render(make(), SplatRasterizer(W, H, device="cuda:0"), cam)[0].clone()
    noise = torch.randn((3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
    target = (frame + 0.1 * noise).clamp_(0.0, 1.0)
    k = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(k * k) / 4.5)
    g = (g / g.sum()).to(torch.float32)
    window2d = (g[:, None] * g[None, :])[None, None].expand(3, 1, 11, 11).contiguous().to(dev)
    composed = torch_ssim_loss(window2d)

    # ---- the loss alone ----
    L = _capi.lib()
    scratch = torch.empty(L.gsr_photo_loss_scratch_bytes(3, W, H), dtype=torch.uint8, device=dev)
    terms, up, grad = torch.empty(3, device=dev), torch.ones((), device=dev), torch.empty_like(frame)
    a = _capi.PhotoLossArgs()
    a.struct_size, a.channels, a.width, a.height, a.lambda_dssim = C.sizeof(_capi.PhotoLossArgs), 3, W, H, LAMBDA
    a.image, a.target, a.scratch, a.out = frame.data_ptr(), target.data_ptr(), scratch.data_ptr(), terms.data_ptr()
    a.dL_dloss, a.dL_dimage, a.want_backward = up.data_ptr(), grad.data_ptr(), 1
    a.stream = torch.cuda.current_stream(dev).cuda_stream
    quiet = _capi.PhotoLossArgs()
    C.memmove(C.byref(quiet), C.byref(a), C.sizeof(_capi.PhotoLossArgs))
    quiet.want_backward = 0
    forward = lambda args=a: _capi.check(L.gsr_photo_loss_forward(C.byref(args)), "gsr_photo_loss_forward")
    backward = lambda: _capi.check(L.gsr_photo_loss_backward(C.byref(a)), "gsr_photo_loss_backward")
    leaf_f, leaf_t = frame.clone().requires_grad_(True), frame.clone().requires_grad_(True)

    def through(loss_fn, leaf):
        def fn():
            leaf.grad = None
            loss_fn(leaf, target).backward()
        return fn

    m = interleaved({"forward": forward, "forward, no backward to follow": lambda: forward(quiet), "backward": backward,
                     "both": lambda: (forward(), backward()), "fused autograd": through(photometric_loss, leaf_f),
                     "torch autograd": through(composed, leaf_t)})
    with torch.no_grad():
        t_loss, f_loss = float(composed(frame, target)), float(photometric_loss(frame, target))
    # both float32 gradients against the same composition in float64 (not timed)
    leaf_d = frame.double().requires_grad_(True)
    torch_ssim_loss(window2d.double())(leaf_d, target.double()).backward()
    scale = leaf_d.grad.abs().max()
    e_fused, e_torch = (float((t.grad.double() - leaf_d.grad).abs().max() / scale) for t in (leaf_f, leaf_t))
    out.append(f"loss: fused {f_loss:.7f}, torch composition {t_loss:.7f}; gradient against the composition in float64, of max|grad|:"
               f" fused {e_fused:.1e}, torch float32 {e_torch:.1e}")
    del leaf_d
    out.append(f"the loss alone ({NEEDED / 1e6:.0f} MB needed: 12 B per image float; {MOVED / 1e6:.0f} MB moved by these kernels: 44 B per float;"
               f" share of the {HBM_PEAK / 1e12:.0f} TB/s peak)")
    rows = (("gsr_photo_loss_forward (want_backward = 1)", "forward", 8 * FLOATS, 20 * FLOATS),
            ("gsr_photo_loss_forward (want_backward = 0)", "forward, no backward to follow", 8 * FLOATS, 8 * FLOATS),
            ("gsr_photo_loss_backward", "backward", 4 * FLOATS, 24 * FLOATS),
            ("forward + backward, the two C calls", "both", NEEDED, MOVED),
            ("photometric_loss() + backward()", "fused autograd", NEEDED, MOVED))
    for what, key, needed, moved in rows:
        out.append(f"  {what:<46s}{m[key]:8.3f} ms   needed {share(m[key], needed)}, moved {share(m[key], moved)}")
    out.append(f"  {'torch composition, forward + backward':<46s}{m['torch autograd']:8.3f} ms")
    ratio = m["torch autograd"] / m["fused autograd"]
    out.append(f"  the torch composition takes {ratio:.1f} x the time of photometric_loss() + backward()"
               + ("" if ratio > 1.0 else ": THE FUSED LOSS IS NOT FASTER"))
    out.append("  (the fused kernels are bound by their VALU work, not by HBM: without contraction a pixel is about 400 float32"
               " operations in the forward's two passes, halo rows included, and 200 in the backward's)")
    del leaf_f, leaf_t
    torch.cuda.empty_cache()

    # ---- the whole step (a rate of 1e-6: the frame stays the frame) ----
    losses = {"L1, (color - target).abs().mean()": lambda color: (color - target).abs().mean(),
              "torch composition": lambda color: composed(color, target),
              "photometric_loss": lambda color: photometric_loss(color, target)}
    steps = {}
    for name, loss_fn in losses.items():
        params, rast, slot = make(), SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
        opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)

        def step(params=params, rast=rast, slot=slot, opt=opt, loss_fn=loss_fn):
            opt.zero_grad(set_to_none=True)
            loss_fn(render(params, rast, cam, radii_slot=slot)[0]).backward()
            opt.step(slot.radii)
        steps[name] = step
    wm = interleaved(steps)
    base = wm["L1, (color - target).abs().mean()"]
    out.append("one training step: render() + loss + backward() + GaussianAdam.step(radii)")
    for name in losses:
        out.append(f"  {name:<46s}{wm[name]:8.3f} ms" + (f" ({wm[name] - base:+.3f} ms)" if wm[name] != base else ""))
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
