"""What the depth distortion map costs (gsr_distortion_forward / gsr_distortion_backward, include/gsrast_amd_distortion.h) on the
bench frame, 1920 x 1080, one GPU. Three measurements, reported and not asserted:
  1. both kernels, for power 2 and 1 (the library's stage_ms, and the whole call by device events), beside the feature pass at
     C = 1 (render_features / features_backward / backward(features=...)) and the render backward of the same frame;
  2. the training step of INTEGRATION.md 2a with the distortion term beside the photometric loss, and without;
  3. the default step (no distortion) through this tree's library and through the parent commit's — built from a checkout of
     that commit (python -m gsrast_amd.build there) and named with --parent-lib; loaded beside this tree's into the same process,
     the two interleaved, as scripts/features_cost.py does. Without --parent-lib the row says "not measured".
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
Usage: python scripts/distortion_cost.py [--reps N] [--splats N] [--parent-lib PATH] [--out FILE] [--only-passes]
(profiles/distortion_cost.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from features_cost import finish, fmt, interleaved, stats, timed  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
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
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_distortion_forward"), "--parent-lib exports gsr_distortion_forward: it is not the parent commit's"
    return P


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    out = [f"distortion map cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    this_lib = _capi.lib()
    gen = torch.Generator().manual_seed(7)

    # ---- 1. the passes beside the feature pass at C = 1 and the render backward ----
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    n = r.num_gaussians
    zeros = torch.zeros((3, H, W), device=dev)
    g3 = torch.randn((3, H, W), generator=gen).to(dev)
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam)
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan {r.last_plan}")
    view = torch.from_numpy(np.asarray(cam.view, np.float32).reshape(-1)).to(dev)
    m3 = r.means3D
    z = ((m3[:, 0] * view[2] + m3[:, 1] * view[6]) + (m3[:, 2] * view[10] + view[14])).contiguous()
    F1 = z[:, None].contiguous()
    G = torch.randn((H, W), generator=gen).to(dev)
    dmap, fmap = torch.empty((H, W), device=dev), torch.empty((1, H, W), device=dev)
    dV, dF = torch.empty((n,), device=dev), torch.empty((n, 1), device=dev)

    def stage(fn, attr):
        def run():
            fn()
            return getattr(r, attr)
        return run
    fns = {"backward": lambda: timed(lambda: r.backward(g3, sync=False)),
           "backward_stage": stage(lambda: r.backward(g3, profile=True), "last_backward_ms"),
           "f_fwd_stage": stage(lambda: r.render_features(F1, into=fmap, profile=True), "last_features_ms"),
           "f_bwd_stage": stage(lambda: r.features_backward(F1, G[None], into=dF, profile=True), "last_features_ms"),
           "f_joint_stage": stage(lambda: r.backward(zeros, features=(F1, G[None]), profile=True), "last_features_ms"),
           "f_joint": lambda: timed(lambda: r.backward(zeros, features=(F1, G[None]), sync=False))}
    for q in (2, 1):
        r.render_distortion(z, power=q)
        mom = r._distortion_moments[2]
        fns[f"d_fwd_stage{q}"] = stage(lambda q=q: r.render_distortion(z, power=q, into=dmap, profile=True), "last_distortion_ms")
        fns[f"d_fwd{q}"] = lambda q=q: timed(lambda: r.render_distortion(z, power=q, into=dmap, sync=False))
        fns[f"d_bwd_stage{q}"] = stage(lambda q=q, mom=mom: r.distortion_backward(z, G, power=q, moments=mom, into=dV, profile=True), "last_distortion_ms")
        fns[f"d_bwd{q}"] = lambda q=q, mom=mom: timed(lambda: r.distortion_backward(z, G, power=q, moments=mom, into=dV, sync=False))
        fns[f"d_joint_stage{q}"] = stage(lambda q=q, mom=mom: r.backward(zeros, distortion=(z, G, q, mom), profile=True), "last_distortion_ms")
        fns[f"d_joint{q}"] = lambda q=q, mom=mom: timed(lambda: r.backward(zeros, distortion=(z, G, q, mom), sync=False))
    res = interleaved(fns)
    s = {k: stats([sum(x) if isinstance(x, tuple) else x for x in v]) for k, v in res.items()}
    out.append(f"one complete backward() (double sums, every output): the whole call {fmt(s['backward'])}; its kernels (render + chain) {fmt(s['backward_stage'])}")
    out.append("the feature pass at C = 1 (values = view depth)")
    out.append(f"  render_features, the kernel                          {fmt(s['f_fwd_stage'])}")
    out.append(f"  features_backward (frozen geometry), the kernels     {fmt(s['f_bwd_stage'])}")
    out.append(f"  backward(features=...): gsr_features_backward        {fmt(s['f_joint_stage'])}")
    out.append(f"  backward(features=...), the whole call               {fmt(s['f_joint'])}")
    for q in (2, 1):
        out.append(f"the distortion pass, power {q} (values = view depth)")
        out.append(f"  render_distortion, the kernel                        {fmt(s[f'd_fwd_stage{q}'])}")
        out.append(f"  render_distortion, the whole call                    {fmt(s[f'd_fwd{q}'])}")
        out.append(f"  distortion_backward (frozen geometry), the kernels   {fmt(s[f'd_bwd_stage{q}'])}")
        out.append(f"  distortion_backward, the whole call                  {fmt(s[f'd_bwd{q}'])}")
        out.append(f"  backward(distortion=...): gsr_distortion_backward    {fmt(s[f'd_joint_stage{q}'])}")
        out.append(f"  backward(distortion=...), the whole call             {fmt(s[f'd_joint{q}'])}")
    del r, fns
    torch.cuda.empty_cache()
    if "--only-passes" in sys.argv:
        return finish(out)

    # ---- 2. the training step of INTEGRATION.md 2a, with and without the distortion term ----
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    dens = DensityStats(params.num_gaussians, dev)

    def make_step(rs, slot, with_distortion):
        def step():
            opt.zero_grad(set_to_none=True)
            if with_distortion:
                color, _, _, dist = render(params, rs, cam, radii_slot=slot, distortion="depth")
                (photometric_loss(color, target) + 100.0 * dist.mean()).backward()
            else:
                color, _, _ = render(params, rs, cam, radii_slot=slot)
                photometric_loss(color, target).backward()
            opt.step(slot.radii)
            dens.update(slot, W, H)
        return step
    steps = {}
    for name, wd in (("no distortion (a)", False), ("distortion=\"depth\" (a)", True), ("no distortion (b)", False),
                     ("distortion=\"depth\" (b)", True)):
        steps[name] = lambda step=make_step(rast, FrameSlot(), wd): timed(step)
    res = interleaved(steps)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii) + DensityStats.update()"
               " [+ 100 x the mean of the distortion map of the view depth, power 2]")
    med = {}
    for name in steps:
        m = stats(res[name])
        med[name] = m[0]
        out.append(f"  {name:<34s}{fmt(m)}")
    plain = 0.5 * (med["no distortion (a)"] + med["no distortion (b)"])
    with_d = 0.5 * (med["distortion=\"depth\" (a)"] + med["distortion=\"depth\" (b)"])
    out.append(f"  with the distortion term against without: {with_d - plain:+.3f} ms (the torch operations that form z and its gradient "
               f"included); equal configurations differ by {abs(med['no distortion (a)'] - med['no distortion (b)']):.3f} ms")

    # ---- 3. the default step against the parent commit's library ----
    out.append("the default step (no distortion) through this tree's library and the parent commit's")
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
        out.append(f"  this tree {mine:.3f} ms against the parent {parent:.3f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own quartiles "
                   f"{lo:.3f} .. {hi:.3f} ms ({1e3 * (hi - lo):.1f} us): {'inside' if lo <= mine <= hi else 'OUTSIDE'}")
    else:
        out.append("  parent commit: not measured (no --parent-lib)")
    finish(out)


if __name__ == "__main__":
    main()
