"""What the gradient of the accumulated opacity costs (gsr_backward_alpha, include/gsrast_amd_opacity.h) on the bench frame, 1920 x 1080, one
GPU. Four measurements:
  1. gsr_backward of the parent commit — its library, built from a checkout of that commit (python -m gsrast_amd.build there)
     and named with --parent-lib; loaded beside this tree's into the same process and called with the same arguments (the
     struct is the same). Entered twice, as two configurations: the distance between their medians is the
     run-to-run spread a difference has to be held against. Without --parent-lib the row says "not measured".
  2. this tree's gsr_backward (gsr_backward_alpha with a NULL gradient),
  3. this tree's gsr_backward_alpha with the gradient,
     all through the C entry point with GSR_FLAG_PROFILE (the library's own events around the render backward and the chain)
     and, without the flag, device events around the whole call;
  4. the training step of INTEGRATION.md 2a — render() + photometric_loss + backward() + GaussianAdam.step(radii) — as it is
     (entered twice: what two equal configurations differ by),
     with opacity_grad=True and nothing on the map (no gradient reaches the backward: the call is the one above), and with a
     mask loss on it (the loss's own torch kernels included).
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
The alpha term reads one float per pixel: 4 W H = 8.3 MB at this size, once. (The kernel's per-pixel inputs together —
n_contrib, final_t, three planes of dL_dout_color — are 41.5 MB.)
Usage: python scripts/alpha_grad_cost.py [--reps N] [--splats N] [--parent-lib PATH] [--out FILE]   (profiles/alpha_grad_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s (spec)


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 40)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)
PARENT = _arg("--parent-lib", None, str)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def interleaved(fns, reps=REPS, warm=5):
    """name -> list of what fn returned (a time, or a tuple of times), one per round; the order rotates with the round."""
    names = list(fns)
    for _ in range(warm):
        for k in names:
            fns[k]()
    torch.cuda.synchronize()
    got = {k: [] for k in names}
    for i in range(reps):
        for k in names[i % len(names):] + names[:i % len(names)]:
            got[k].append(fns[k]())
    return got


def stats(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(np.percentile(v, 25)), float(np.percentile(v, 75))


def captured_backward_args(r, dl, **kw):
    """The gsr_backward_args of r.backward(dl, **kw), copied while the call is made (the arrays it points to are this
    object's buffers: they stay where they are for the calls that replay it)."""
    held = {}
    real = _capi.call

    def spy(name, *args, **kwargs):
        if name == "gsr_backward":
            a = _capi.BackwardArgs()
            C.memmove(C.byref(a), args[0], C.sizeof(_capi.BackwardArgs))
            held["args"] = a
        return real(name, *args, **kwargs)
    _capi.call = spy
    try:
        r.backward(dl, **kw)
    finally:
        _capi.call = real
    return held["args"]


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    out = [f"alpha gradient cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    gen = torch.Generator().manual_seed(7)
    dl = torch.randn((3, H, W), generator=gen).to(dev)
    ga = torch.randn((H, W), generator=gen).to(dev)
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam)
    out.append(f"N = {r.num_gaussians}, R = {r.last_num_rendered}, plan {r.last_plan}")

    # ---- gsr_backward: the same arguments through this tree's library and the parent's ----
    L = _capi.lib()
    base = captured_backward_args(r, dl)                  # wide sums, every output: backward()'s defaults
    with_alpha = lambda ref: L.gsr_backward_alpha(ref, ga.data_ptr())
    calls = {"this tree, dL_dout_alpha = NULL": (L.gsr_backward, base), "this tree, dL_dout_alpha given": (with_alpha, base)}
    if PARENT:
        P = C.CDLL(os.path.abspath(PARENT))
        P.gsr_backward.restype, P.gsr_backward.argtypes = C.c_int, [C.POINTER(_capi.BackwardArgs)]
        calls = {"parent commit (a)": (P.gsr_backward, base), **calls, "parent commit (b)": (P.gsr_backward, base)}

    def profiled(fn, a):
        def run():
            a.flags |= _capi.GSR_FLAG_PROFILE
            _capi.check(fn(C.byref(a)), "gsr_backward")
            return float(a.stage_ms[0]), float(a.stage_ms[1])
        return run

    def whole(fn, a):
        def run():
            a.flags &= ~_capi.GSR_FLAG_PROFILE
            return timed(lambda: _capi.check(fn(C.byref(a)), "gsr_backward"))
        return run
    with torch.cuda.device(dev):
        stages = interleaved({k: profiled(*v) for k, v in calls.items()})
        totals = interleaved({k: whole(*v) for k, v in calls.items()})
    out.append("gsr_backward (double sums, every output): render backward and chain by the library's events, the whole call by device events")
    med, quart = {}, {}
    for k in calls:
        rb, ch, tot = stats([s[0] for s in stages[k]]), stats([s[1] for s in stages[k]]), stats(totals[k])
        med[k] = (rb[0], tot[0], rb[2] - rb[1], tot[2] - tot[1])
        quart[k] = ((rb[1], rb[2]), (tot[1], tot[2]))
        out.append(f"  {k:<34s} render backward {rb[0]:7.4f} ms ({rb[1]:.4f} .. {rb[2]:.4f})   chain {ch[0]:7.4f} ms   "
                   f"call {tot[0]:7.4f} ms ({tot[1]:.4f} .. {tot[2]:.4f})")
    null, given = med["this tree, dL_dout_alpha = NULL"], med["this tree, dL_dout_alpha given"]
    if PARENT:
        pa, pb = med["parent commit (a)"], med["parent commit (b)"]
        for what, i in (("render backward", 0), ("whole call", 1)):
            # the parent's own spread: from the lowest first quartile to the highest third quartile of its two configurations
            lo = min(quart["parent commit (a)"][i][0], quart["parent commit (b)"][i][0])
            hi = max(quart["parent commit (a)"][i][1], quart["parent commit (b)"][i][1])
            diff = null[i] - 0.5 * (pa[i] + pb[i])
            out.append(f"  NULL against the parent, {what}: median {1e3 * diff:+.1f} us; the parent's two configurations: medians "
                       f"{1e3 * abs(pa[i] - pb[i]):.1f} us apart, quartiles {lo:.4f} .. {hi:.4f} ms -> the NULL median {null[i]:.4f} ms lies "
                       f"{'within' if lo <= null[i] <= hi else 'OUTSIDE'} them")
    else:
        out.append("  parent commit: not measured (no --parent-lib)")
    extra = 4 * W * H
    for what, i in (("render backward", 0), ("whole call", 1)):
        d = given[i] - null[i]
        out.append(f"  the alpha term, {what}: {1e3 * d:+.1f} us for {extra / 1e6:.2f} MB more read, one float per pixel ({1e6 * extra / HBM_PEAK:.1f} us at the "
                   f"{HBM_PEAK / 1e12:.0f} TB/s peak); interquartile ranges {1e3 * null[i + 2]:.1f} / {1e3 * given[i + 2]:.1f} us")

    # ---- the training step of INTEGRATION.md 2a ----
    del r
    torch.cuda.empty_cache()
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame, _, opacity = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    mask = (opacity > 0.5).to(torch.float32)
    steps = {}
    # (one set of parameters, rasterizer and optimiser for every configuration: separate sets differ by 0.05 ms among themselves)
    params, rast, slot = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    for name, grad, masked in (("as it is (a)", False, False), ("opacity_grad=True, nothing on the map", True, False),
                               ("opacity_grad=True, mask loss |opacity - mask|.mean()", True, True), ("as it is (b)", False, False)):
        def step(grad=grad, masked=masked):
            opt.zero_grad(set_to_none=True)
            color, _, opac = render(params, rast, cam, radii_slot=slot, opacity_grad=grad)
            loss = photometric_loss(color, target)
            if masked:
                loss = loss + (opac - mask).abs().mean()
            loss.backward()
            opt.step(slot.radii)
        steps[name] = lambda step=step: timed(step)
    got = interleaved(steps, warm=3)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii)")
    first = None
    for name in steps:
        m = stats(got[name])
        first = m[0] if first is None else first
        out.append(f"  {name:<54s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})" + (f" ({m[0] - first:+.3f} ms)" if m[0] != first else ""))
    leaf = opacity.clone().requires_grad_(True)

    def mask_loss_alone():
        leaf.grad = None
        (leaf - mask).abs().mean().backward()
    alone = stats(interleaved({"mask": lambda: timed(mask_loss_alone)}, warm=3)["mask"])
    out.append(f"  (the mask loss and its backward alone, torch ops on a leaf map: {alone[0]:.3f} ms)")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
