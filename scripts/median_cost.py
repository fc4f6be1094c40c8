"""What the median map and the per-pixel ids cost (gsr_median_forward / gsr_median_backward, include/gsrast_amd_median.h) on the bench
frame, 1920 x 1080, one GPU. Three measurements and two rules, each against something that is not the code under test:
  1. render_median with values only, with ids, and with `dominant` too; median_backward; pick (one tile row and its
     synchronisation) — the whole Python call by device events — beside render_features at C = 1, twice in the same rounds.
     RULE 1: the values-only forward does strictly less per record than that call (no payload staged, no sums formed), so its median
     must not exceed the upper quartile of that call's own repeats.
  2. the training step of INTEGRATION.md 2a with the normal-consistency term on the expected depth, with it on the median depth
     (normal_consistency(surface_depth=median)), and without the term.
  3. RULE 2: the default step through this tree's library and through the parent commit's — built from a checkout of that commit
     (python -m gsrast_amd.build there) and named with --parent-lib; loaded beside this tree's into the same process, the two
     interleaved. This tree's median must fall inside the parent's own quartiles. Without --parent-lib the row says "not measured".
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
Usage: python scripts/median_cost.py [--reps N] [--splats N] [--parent-lib PATH] [--out FILE] [--only-passes]
(profiles/median_cost.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from features_cost import finish, fmt, interleaved, stats, timed  # noqa: E402
from gsrast_amd import _capi, camera, normals  # noqa: E402
from gsrast_amd.autograd import FrameSlot, GaussianParams, render  # noqa: E402
from gsrast_amd.densify import DensityStats  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 30)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)
PARENT = _arg("--parent-lib", None, str)


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point it has gets this tree's signature."""
    import ctypes as C
    P = C.CDLL(os.path.abspath(path))
    for table in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES,
                  _capi.DISTORTION_SIGNATURES, _capi.NORMALS_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_median_forward"), "--parent-lib exports gsr_median_forward: it is not the parent commit's"
    return P


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    tan = (float(cam.tan_fovx), float(cam.tan_fovy))
    out = [f"median map and per-pixel ids: cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    this_lib = _capi.lib()
    gen = torch.Generator().manual_seed(7)

    # ---- 1. the calls, beside render_features at C = 1 ----
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    n = r.num_gaussians
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam)
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan {r.last_plan}")
    view = torch.from_numpy(np.asarray(cam.view, np.float32).reshape(-1)).to(dev)
    m3 = r.means3D
    z = ((m3[:, 0] * view[2] + m3[:, 1] * view[6]) + (m3[:, 2] * view[10] + view[14])).contiguous()
    one = z.reshape(n, 1).contiguous()
    g = torch.randn((H, W), generator=gen).to(dev)
    bufs = {"map": torch.empty((H, W), device=dev), "ids": torch.empty((H, W), dtype=torch.int32, device=dev),
            "dominant_ids": torch.empty((H, W), dtype=torch.int32, device=dev)}
    feat = torch.empty((1, H, W), device=dev)
    ids = r.render_median(z)["ids"]
    crossed = float((r.map_image_state()["finalT"] <= 0.5).float().mean())
    out.append(f"(threshold 0.5; the transmittance falls through it in {100 * crossed:.1f} % of the pixels, "
               f"{100 * float((ids >= 0).float().mean()):.1f} % blended something)")
    fns = {"features C=1 (a)": lambda: timed(lambda: r.render_features(one, into=feat, sync=False)),
           "values only": lambda: timed(lambda: r.render_median(z, ids=False, out={"map": bufs["map"]}, sync=False)),
           "values and ids": lambda: timed(lambda: r.render_median(z, out={"map": bufs["map"], "ids": bufs["ids"]}, sync=False)),
           "values, ids, dominant": lambda: timed(lambda: r.render_median(z, dominant=True, out=bufs, sync=False)),
           "values only, threshold 0": lambda: timed(lambda: r.render_median(z, threshold=0.0, ids=False, out={"map": bufs["map"]}, sync=False)),
           "features C=1 (b)": lambda: timed(lambda: r.render_features(one, into=feat, sync=False)),
           "backward": lambda: timed(lambda: r.median_backward(ids, g, sync=False)),
           "pick": lambda: timed(lambda: r.pick(W // 2, H // 2))}
    s = {k: stats(v) for k, v in interleaved(fns).items()}
    for k in fns:
        out.append(f"  {k:<34s}{fmt(s[k])}")
    fa, fb = s["features C=1 (a)"], s["features C=1 (b)"]
    hi = max(fa[2], fb[2])
    mine = s["values only"][0]
    out.append(f"  RULE 1: values only {mine:.3f} ms against render_features at C = 1 {0.5 * (fa[0] + fb[0]):.3f} ms (its repeats: medians "
               f"{fa[0]:.3f} and {fb[0]:.3f} ms, quartiles {min(fa[1], fb[1]):.3f} .. {hi:.3f} ms): "
               f"{'not longer: inside' if mine <= hi else 'LONGER: OUTSIDE'}")
    del fns, r, bufs, feat, one, z, g, ids
    torch.cuda.empty_cache()
    if "--only-passes" in sys.argv:
        return finish(out)

    # ---- 2. the training step of INTEGRATION.md 2a: the normal-consistency term on the expected and on the median depth ----
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    dens = DensityStats(params.num_gaussians, dev)

    def make_step(rs, slot, mode):
        def step():
            opt.zero_grad(set_to_none=True)
            if mode == "median":
                color, dmap, omap, nmap, med = render(params, rs, cam, radii_slot=slot, depth=True, opacity_grad=True, normals=True, median="depth")
                (photometric_loss(color, target) + 0.05 * normals.normal_consistency(nmap, dmap, omap, tan, surface_depth=med).mean()).backward()
            elif mode == "expected":
                color, dmap, omap, nmap = render(params, rs, cam, radii_slot=slot, depth=True, opacity_grad=True, normals=True)
                (photometric_loss(color, target) + 0.05 * normals.normal_consistency(nmap, dmap, omap, tan).mean()).backward()
            else:
                color, _, _ = render(params, rs, cam, radii_slot=slot)
                photometric_loss(color, target).backward()
            opt.step(slot.radii)
            dens.update(slot, W, H)
        return step
    steps = {}
    for name, mode in (("no normal term (a)", None), ("expected depth", "expected"), ("median depth", "median"), ("no normal term (b)", None)):
        steps[name] = lambda step=make_step(rast, FrameSlot(), mode): timed(step)
    res = interleaved(steps)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii) + DensityStats.update()"
               " [+ 0.05 x the mean of normal_consistency: depth=True, opacity_grad=True, normals=True[, median=\"depth\" as surface_depth]]")
    med = {}
    for name in steps:
        m = stats(res[name])
        med[name] = m[0]
        out.append(f"  {name:<34s}{fmt(m)}")
    out.append(f"  the term on the median depth against the term on the expected depth: {med['median depth'] - med['expected depth']:+.3f} ms "
               f"(the median pass, its backward and the torch composition of the view depth); against no term: "
               f"{med['median depth'] - 0.5 * (med['no normal term (a)'] + med['no normal term (b)']):+.3f} ms; equal configurations differ by "
               f"{abs(med['no normal term (a)'] - med['no normal term (b)']):.3f} ms")

    # ---- 3. the default step against the parent commit's library ----
    out.append("the default step (no median) through this tree's library and the parent commit's")
    if PARENT:
        P = load_parent(PARENT)

        def through(lib):
            """A step whose every call goes through `lib`: a rasterizer made under it, and the ctypes table pointed at it."""
            _capi._lib = lib
            inner = make_step(SplatRasterizer(W, H, device="cuda:0"), FrameSlot(), None)

            def step():
                _capi._lib = lib
                inner()
            return step
        steps = {"parent commit (a)": through(P), "this tree (a)": through(this_lib), "parent commit (b)": through(P),
                 "this tree (b)": through(this_lib)}
        res = interleaved({k: (lambda fn=fn: timed(fn)) for k, fn in steps.items()}, reps=max(REPS, 40))
        _capi._lib = this_lib
        med, quart = {}, {}
        for name in steps:
            m = stats(res[name])
            med[name], quart[name] = m[0], (m[1], m[2])
            out.append(f"  {name:<34s}{fmt(m)}")
        parent = 0.5 * (med["parent commit (a)"] + med["parent commit (b)"])
        mine = 0.5 * (med["this tree (a)"] + med["this tree (b)"])
        lo = min(quart["parent commit (a)"][0], quart["parent commit (b)"][0])
        hi = max(quart["parent commit (a)"][1], quart["parent commit (b)"][1])
        out.append(f"  RULE 2: this tree {mine:.3f} ms against the parent {parent:.3f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own quartiles "
                   f"{lo:.3f} .. {hi:.3f} ms ({1e3 * (hi - lo):.1f} us): {'inside' if lo <= mine <= hi else 'OUTSIDE'}; equal configurations "
                   f"differ by {1e3 * abs(med['parent commit (a)'] - med['parent commit (b)']):.1f} us (parent) and "
                   f"{1e3 * abs(med['this tree (a)'] - med['this tree (b)']):.1f} us (this tree)")
    else:
        out.append("  parent commit: not measured (no --parent-lib)")
    finish(out)


if __name__ == "__main__":
    main()
