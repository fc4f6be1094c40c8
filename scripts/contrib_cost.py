"""What the per-Gaussian contribution statistics cost (gsr_contribution, include/gsrast_amd_contrib.h) on the bench frame, 1920 x 1080,
one GPU, beside the two existing kernels that walk the same sorted lists, all from one process:
  1. the pass itself — all four outputs, without `dominant`, and weight_max alone — by the library's own events (GSR_FLAG_PROFILE)
     and, without the flag, by device events around the whole call;
  2. the forward blend from the sorted lists (draw(plan="sort", profile=True): the stage "blend"), and the blend of the plan the
     library picks for this frame;
  3. the render backward (backward(profile=True): stage_ms[0]);
  4. the training step of INTEGRATION.md 2a — render() + photometric_loss + backward() + GaussianAdam.step(radii) — as it is
     (entered twice: what two equal configurations differ by) and with stats.update(rast) between render() and backward().
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
The atomics the pass issues are bounded from the frame's own state: per array one per (tile, staged record that blended anywhere
in the tile) — at most the records the tiles walk (sum over tiles of the largest n_contrib), at least the Gaussians some pixel
blended; `dominant` adds at most one per pixel with a contributor.
Usage: python scripts/contrib_cost.py [--reps N] [--splats N] [--out FILE]   (profiles/contrib_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.contrib import WHAT, ContributionStats, contribution_args  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 40)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def interleaved(fns, reps=REPS, warm=5):
    """name -> list of what fn returned, one per round; the order rotates with the round."""
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


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    out = [f"contribution statistics cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    dl = torch.randn((3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam)
    auto_plan = r.last_plan
    n = r.num_gaussians
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan picked for this frame: {auto_plan}")

    # ---- the pass beside the forward blend and the render backward, over the same sorted lists ----
    r.draw(cam, plan="sort")
    full = ContributionStats(n, dev)
    arrays = {k: torch.zeros_like(t) for k, t in full.raw.items()}
    subsets = {"all four outputs": WHAT, "without dominant": WHAT[:3], "weight_max alone": ("weight_max",)}
    L = _capi.lib()

    def contribution(names, profile):
        a = contribution_args(r, r.last_receipt, "gscuda", {k: arrays[k].data_ptr() for k in names})

        def run():
            if profile:
                a.flags |= _capi.GSR_FLAG_PROFILE
                _capi.check(L.gsr_contribution(C.byref(a)), "gsr_contribution")
                return float(a.stage_ms)
            a.flags &= ~_capi.GSR_FLAG_PROFILE
            return timed(lambda: _capi.check(L.gsr_contribution(C.byref(a)), "gsr_contribution"))
        return run

    def forward_blend(plan):
        def run():
            r.draw(cam, plan=plan, profile=True)
            return r.last_stage_ms["blend"]
        return run

    def render_backward():
        r.backward(dl, profile=True)
        return r.last_backward_ms[0]
    with torch.cuda.device(dev):
        fns = {f"gsr_contribution, {k}": contribution(v, True) for k, v in subsets.items()}
        fns.update({f"gsr_contribution, {k} (whole call)": contribution(v, False) for k, v in subsets.items()})
        fns["forward blend from the sorted lists (plan=sort)"] = forward_blend("sort")
        fns["render backward (stage_ms[0])"] = render_backward
        got = interleaved(fns)
        blend_auto = stats(interleaved({"b": forward_blend("auto")})["b"])
        r.draw(cam, plan="sort")
    med = {}
    for k in fns:
        m = stats(got[k])
        med[k] = m[0]
        out.append(f"  {k:<52s}{m[0]:8.4f} ms ({m[1]:.4f} .. {m[2]:.4f})")
    out.append(f"  {'forward blend of the plan picked (' + auto_plan + ')':<52s}{blend_auto[0]:8.4f} ms ({blend_auto[1]:.4f} .. {blend_auto[2]:.4f})")
    p = med["gsr_contribution, all four outputs"]
    fb, rb = med["forward blend from the sorted lists (plan=sort)"], med["render backward (stage_ms[0])"]
    out.append(f"  the pass (all four) is {p / fb:.2f} x the forward blend from the same lists and {p / rb:.2f} x the render backward; "
               f"dominant costs {1e3 * (p - med['gsr_contribution, without dominant']):+.1f} us, the sums and counts "
               f"{1e3 * (med['gsr_contribution, without dominant'] - med['gsr_contribution, weight_max alone']):+.1f} us over weight_max alone")

    # ---- the atomics, bounded from the frame's state ----
    for t in arrays.values():
        t.zero_()
    a = contribution_args(r, r.last_receipt, "gscuda", {k: t.data_ptr() for k, t in arrays.items()})
    _capi.call("gsr_contribution", C.byref(a), device=dev)
    torch.cuda.synchronize()
    im = r.map_image_state()
    gx, gy = (W + 15) // 16, (H + 15) // 16
    nc = torch.zeros((gy * 16, gx * 16), dtype=torch.int64, device=dev)
    nc[:H, :W] = im["nContrib"].to(torch.int64)
    walked = int(nc.view(gy, 16, gx, 16).amax(dim=(1, 3)).sum())
    blended = int((arrays["pixels"] > 0).sum())
    lit = int((im["nContrib"] > 0).sum())
    pairs = int(arrays["pixels"].sum())
    out.append(f"  records the tiles walk (sum over tiles of the largest n_contrib): {walked}; (pixel, record) pairs blended: {pairs} "
               f"({pairs / max(1, walked):.1f} per walked record: what the on-chip reduction folds into one atomic); Gaussians blended "
               f"somewhere: {blended}; pixels with a contributor: {lit}")
    lo, hi = 3 * blended, 3 * walked + lit
    out.append(f"  global integer atomics of one pass (all four outputs): between {lo} and {hi} (3 per tile and blended record, at most one "
               f"per lit pixel for dominant); in {p:.4f} ms that is between {lo / p / 1e6:.2f} and {hi / p / 1e6:.2f} G atomics/s, "
               f"{8 * hi / p / 1e9:.3f} TB/s of added bytes at most: not what bounds the pass unless the figure nears the float-atomic rate "
               f"of 1.3 TB/s")

    # ---- the training step of INTEGRATION.md 2a ----
    del r
    torch.cuda.empty_cache()
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    gen = torch.Generator().manual_seed(7)
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast, slot = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    acc = ContributionStats(n, dev)
    steps = {}
    for name, update in (("as it is (a)", False), ("with stats.update(rast) before backward()", True), ("as it is (b)", False)):
        def step(update=update):
            opt.zero_grad(set_to_none=True)
            color = render(params, rast, cam, radii_slot=slot)[0]
            loss = photometric_loss(color, target)
            if update:
                acc.update(rast)
            loss.backward()
            opt.step(slot.radii)
        steps[name] = lambda step=step: timed(step)
    got = interleaved(steps, warm=3)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii)")
    first = None
    for name in steps:
        m = stats(got[name])
        first = m[0] if first is None else first
        out.append(f"  {name:<52s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})" + (f" ({m[0] - first:+.3f} ms)" if m[0] != first else ""))
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
