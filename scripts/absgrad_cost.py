"""What the absolute screen-space gradient costs (gsr_absgrad, include/gsrast_amd_absgrad.h) on the bench frame, 1920 x 1080, one
GPU. Three measurements:
  1. the pass beside the render backward of the same frame: gsr_absgrad's stage_ms (the walk and the rounding kernel together,
     the library's own events) and gsr_backward's stage_ms[0] (the render backward) and [1] (the chain), through
     SplatRasterizer.absgrad / .backward with profile=True, interleaved; and both calls whole, by device events;
  2. the training step of INTEGRATION.md 2a — render() + photometric_loss + backward() + GaussianAdam.step(radii) +
     DensityStats.update() — with FrameSlot(absgrad=True) and with a plain FrameSlot, each entered twice (what two equal
     configurations differ by);
  3. the default step (a plain FrameSlot) through this tree's library and through the parent commit's — built from a checkout
     of that commit (python -m gsrast_amd.build there) and named with --parent-lib; loaded beside this tree's into the same
     process, the two interleaved. The difference is held against the parent's own inter-quartile spread. Without --parent-lib
     the row says "not measured".
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
Usage: python scripts/absgrad_cost.py [--reps N] [--splats N] [--parent-lib PATH] [--out FILE]   (profiles/absgrad_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import FrameSlot, GaussianParams, render  # noqa: E402
from gsrast_amd.densify import DensityStats  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080


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


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point it has gets this tree's signature."""
    P = C.CDLL(os.path.abspath(path))
    for table in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_absgrad"), "--parent-lib exports gsr_absgrad: it is not the parent commit's"
    return P


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    out = [f"absgrad cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    this_lib = _capi.lib()
    gen = torch.Generator().manual_seed(7)
    dl = torch.randn((3, H, W), generator=gen).to(dev)

    # ---- 1. the pass beside the render backward ----
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam)
    n = r.num_gaussians
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan {r.last_plan}")
    into = torch.empty((n, 2), dtype=torch.float32, device=dev)

    def absgrad_profiled():
        r.absgrad(dl, into=into, profile=True)
        return r.last_absgrad_ms

    def backward_profiled():
        r.backward(dl, profile=True)
        return r.last_backward_ms
    stages = interleaved({"absgrad": absgrad_profiled, "backward": backward_profiled})
    whole = interleaved({"absgrad": lambda: timed(lambda: r.absgrad(dl, into=into, sync=False)),
                         "backward": lambda: timed(lambda: r.backward(dl, sync=False))})
    ab, rb, ch = stats(stages["absgrad"]), stats([s[0] for s in stages["backward"]]), stats([s[1] for s in stages["backward"]])
    out.append("the pass beside gsr_backward of the same frame (double sums, every output), by the library's events")
    out.append(f"  gsr_absgrad, walk + rounding kernel   {ab[0]:7.4f} ms ({ab[1]:.4f} .. {ab[2]:.4f})")
    out.append(f"  gsr_backward, render backward         {rb[0]:7.4f} ms ({rb[1]:.4f} .. {rb[2]:.4f})")
    out.append(f"  gsr_backward, chain                   {ch[0]:7.4f} ms ({ch[1]:.4f} .. {ch[2]:.4f})")
    wa, wb = stats(whole["absgrad"]), stats(whole["backward"])
    out.append(f"  the whole calls through Python, by device events: absgrad {wa[0]:.4f} ms ({wa[1]:.4f} .. {wa[2]:.4f}), "
               f"backward {wb[0]:.4f} ms ({wb[1]:.4f} .. {wb[2]:.4f})")
    out.append(f"  the pass is {ab[0] / rb[0]:.2f} of the render backward")
    got = into.clone()
    signed = r.backward(dl, outputs=("dL_dmean2D", "dL_dconic_opacity"))["dL_dmean2D"]
    seen = got.sum(dim=1) > 0
    ratio = (got[seen].norm(dim=1) / signed[seen].norm(dim=1).clamp_min(1e-30)).median()
    out.append(f"  {int(seen.sum())} Gaussians with a share ({int((signed != 0).any(dim=1).sum())} with a non-zero dL_dmean2D); "
               f"median |abs| / |signed| = {float(ratio):.2f} (white-noise dL_dout)")
    # the rounding kernel alone: a frame drawn with an empty band of tile rows has no walk, the call is that kernel
    r.draw(cam, tile_rows=(1, 1))

    def finish_profiled():
        r.absgrad(dl, into=into, tile_rows=(1, 1), profile=True)
        return r.last_absgrad_ms
    fin = stats(interleaved({"finish": finish_profiled})["finish"])
    out.append(f"  the rounding kernel alone (an empty band: 16 N bytes read, 8 N written) {fin[0]:.4f} ms ({fin[1]:.4f} .. {fin[2]:.4f}): the walk is "
               f"about {ab[0] - fin[0]:.3f} ms, {(ab[0] - fin[0]) / rb[0]:.2f} of the render backward, whose own rounding is part of the chain")
    out.append("  (the walk keeps two sums for twelve and is not six times quicker: both walks are bound by what a wave issues per record and "
               "strip — the power, the exponential in double, the tests, the reciprocal — not by the sums or their atomics)")
    del r, into
    torch.cuda.empty_cache()

    # ---- 2. the training step of INTEGRATION.md 2a, with and without the pass ----
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    dens = DensityStats(params.num_gaussians, dev)

    def make_step(rs, slot, absgrad):
        def step():
            opt.zero_grad(set_to_none=True)
            color, _, _ = render(params, rs, cam, radii_slot=slot)
            photometric_loss(color, target).backward()
            opt.step(slot.radii)
            dens.update(slot, W, H, absgrad=absgrad)
        return step
    steps = {}
    for name, absgrad in (("FrameSlot() (a)", False), ("FrameSlot(absgrad=True) (a)", True), ("FrameSlot() (b)", False),
                          ("FrameSlot(absgrad=True) (b)", True)):
        steps[name] = lambda step=make_step(rast, FrameSlot(absgrad=absgrad), absgrad): timed(step)
    res = interleaved(steps, warm=3)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii) + DensityStats.update()")
    med = {}
    for name in steps:
        m = stats(res[name])
        med[name] = m[0]
        out.append(f"  {name:<32s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
    plain = 0.5 * (med["FrameSlot() (a)"] + med["FrameSlot() (b)"])
    with_abs = 0.5 * (med["FrameSlot(absgrad=True) (a)"] + med["FrameSlot(absgrad=True) (b)"])
    out.append(f"  with absgrad against without: {with_abs - plain:+.3f} ms; equal configurations differ by "
               f"{abs(med['FrameSlot() (a)'] - med['FrameSlot() (b)']):.3f} / "
               f"{abs(med['FrameSlot(absgrad=True) (a)'] - med['FrameSlot(absgrad=True) (b)']):.3f} ms")

    # ---- 3. the default step against the parent commit's library ----
    out.append("the default step (a plain FrameSlot) through this tree's library and the parent commit's")
    if PARENT:
        P = load_parent(PARENT)

        def through(lib):
            """A step whose every call goes through `lib`: a rasterizer made under it, and the ctypes table pointed at it."""
            _capi._lib = lib
            inner = make_step(SplatRasterizer(W, H, device="cuda:0"), FrameSlot(), False)

            def step():
                _capi._lib = lib
                inner()
            return step
        steps = {"parent commit (a)": through(P), "this tree (a)": through(this_lib), "parent commit (b)": through(P),
                 "this tree (b)": through(this_lib)}
        res = interleaved({k: (lambda fn=fn: timed(fn)) for k, fn in steps.items()}, warm=3)
        _capi._lib = this_lib
        med, quart = {}, {}
        for name in steps:
            m = stats(res[name])
            med[name], quart[name] = m[0], (m[1], m[2])
            out.append(f"  {name:<32s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
        parent = 0.5 * (med["parent commit (a)"] + med["parent commit (b)"])
        mine = 0.5 * (med["this tree (a)"] + med["this tree (b)"])
        lo = min(quart["parent commit (a)"][0], quart["parent commit (b)"][0])
        hi = max(quart["parent commit (a)"][1], quart["parent commit (b)"][1])
        out.append(f"  this tree {mine:.3f} ms against the parent {parent:.3f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own quartiles "
                   f"{lo:.3f} .. {hi:.3f} ms ({1e3 * (hi - lo):.1f} us): {'inside' if lo <= mine <= hi else 'OUTSIDE'}")
    else:
        out.append("  parent commit: not measured (no --parent-lib)")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
