"""What N-channel feature maps cost (gsr_features_forward / gsr_features_backward, include/gsrast_amd_features.h) on the bench
frame, 1920 x 1080, one GPU. Four measurements:
  1. at C = 3, 16 and 64: render_features (the library's stage_ms, and the whole call by device events) against what a user had
     before — ceil(C / 3) complete draw(colors_precomp=...) calls; features_backward (frozen geometry) and
     backward(zeros, features=...) (features + geometry in one chain) against ceil(C / 3) complete backward() calls;
  2. the training step of INTEGRATION.md 2a with a 16-channel feature loss beside the photometric loss, and without;
  3. the default step (no features) through this tree's library and through the parent commit's — built from a checkout of that
     commit (python -m gsrast_amd.build there) and named with --parent-lib; loaded beside this tree's into the same process, the
     two interleaved. The difference is held against the parent's own inter-quartile spread. Without --parent-lib the row says
     "not measured";
  4. (tuning) with GSR_LIB_TAG naming a build made with GSR_DEFINES=-DGSR_FEATURES_CHUNK=K, section 1 is that build's: how the
     chunk width was chosen.
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
Usage: python scripts/features_cost.py [--reps N] [--splats N] [--channels 3,16,64] [--parent-lib PATH] [--out FILE] [--only-passes]
(profiles/features_cost.txt)"""
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


REPS = _arg("--reps", 30)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)
PARENT = _arg("--parent-lib", None, str)
CHANNELS = tuple(int(c) for c in _arg("--channels", "3,16,64", str).split(","))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def interleaved(fns, reps=REPS, warm=3):
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


def fmt(m):
    return f"{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})"


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point it has gets this tree's signature."""
    P = C.CDLL(os.path.abspath(path))
    for table in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_features_forward"), "--parent-lib exports gsr_features_forward: it is not the parent commit's"
    return P


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    tag = os.environ.get("GSR_LIB_TAG", "")
    out = [f"feature maps cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds"
           + (f", library build '{tag}'" if tag else f", chunk widths {_capi.GSR_FEATURES_CHUNK_NARROW} (C <= {_capi.GSR_FEATURES_CHUNK_NARROW}) / {_capi.GSR_FEATURES_CHUNK}"), f"bench frame ({label})"]
    this_lib = _capi.lib()
    gen = torch.Generator().manual_seed(7)

    # ---- 1. the passes against ceil(C / 3) complete calls ----
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    n = r.num_gaussians
    colours = torch.rand((n, 3), generator=gen).to(dev)
    zeros = torch.zeros((3, H, W), device=dev)
    g3 = torch.randn((3, H, W), generator=gen).to(dev)
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam, colors_precomp=colours)
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan {r.last_plan}")
    base = interleaved({"draw": lambda: timed(lambda: r.draw(cam, colors_precomp=colours, sync=False)),
                        "backward": lambda: timed(lambda: r.backward(g3, sync=False))})
    r.draw(cam, colors_precomp=colours)
    draw1, back1 = stats(base["draw"]), stats(base["backward"])
    out.append(f"one complete draw(colors_precomp=...) {fmt(draw1)}; one complete backward() (double sums, every output) {fmt(back1)}")
    for c in CHANNELS:
        F = torch.randn((n, c), generator=gen).to(dev)
        G = torch.randn((c, H, W), generator=gen).to(dev)
        fmap = torch.empty((c, H, W), device=dev)
        dF = torch.empty((n, c), device=dev)
        calls = -(-c // 3)

        def fwd_stage():
            r.render_features(F, into=fmap, profile=True)
            return r.last_features_ms

        def bwd_stage():
            r.features_backward(F, G, into=dF, profile=True)
            return r.last_features_ms

        def joint_stage():
            r.backward(zeros, features=(F, G), profile=True)
            return r.last_features_ms
        res = interleaved({"fwd_stage": fwd_stage, "bwd_stage": bwd_stage, "joint_stage": joint_stage,
                           "fwd": lambda: timed(lambda: r.render_features(F, into=fmap, sync=False)),
                           "bwd": lambda: timed(lambda: r.features_backward(F, G, into=dF, sync=False)),
                           "joint": lambda: timed(lambda: r.backward(zeros, features=(F, G), sync=False)),
                           "plain": lambda: timed(lambda: r.backward(zeros, sync=False))})
        s = {k: stats(v) for k, v in res.items()}
        out.append(f"C = {c}: the baseline is {calls} complete call(s) each way")
        out.append(f"  render_features, the kernel                       {fmt(s['fwd_stage'])}")
        out.append(f"  render_features, the whole call                   {fmt(s['fwd'])}   against {calls} x draw = {calls * draw1[0]:.3f} ms: "
                   f"{calls * draw1[0] / s['fwd'][0]:.2f} x")
        out.append(f"  features_backward (frozen geometry), the kernels  {fmt(s['bwd_stage'])}")
        out.append(f"  features_backward, the whole call                 {fmt(s['bwd'])}   against {calls} x backward = {calls * back1[0]:.3f} ms: "
                   f"{calls * back1[0] / s['bwd'][0]:.2f} x")
        out.append(f"  backward(features=...): gsr_features_backward     {fmt(s['joint_stage'])}")
        out.append(f"  backward(features=...), the whole call            {fmt(s['joint'])}   (backward() alone {s['plain'][0]:.3f} ms) against "
                   f"{calls} x backward = {calls * back1[0]:.3f} ms: {calls * back1[0] / s['joint'][0]:.2f} x")
        del F, G, fmap, dF
        r._bw.scratch.pop("feature_sums_f64", None)
        torch.cuda.empty_cache()
    del r
    torch.cuda.empty_cache()
    if "--only-passes" in sys.argv:
        return finish(out)

    # ---- 2. the training step of INTEGRATION.md 2a, with and without a feature loss ----
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    dens = DensityStats(params.num_gaussians, dev)
    cf = 16
    feats = torch.nn.Parameter(torch.randn((params.num_gaussians, cf), generator=gen).to(dev))
    opt_f = torch.optim.Adam([feats], lr=1e-6)
    f_target = torch.randn((cf, H, W), generator=gen).to(dev)

    def make_step(rs, slot, with_features):
        def step():
            opt.zero_grad(set_to_none=True)
            if with_features:
                opt_f.zero_grad(set_to_none=True)
                color, _, _, fmap = render(params, rs, cam, radii_slot=slot, features=feats)
                (photometric_loss(color, target) + (fmap - f_target).abs().mean()).backward()
                opt_f.step()
            else:
                color, _, _ = render(params, rs, cam, radii_slot=slot)
                photometric_loss(color, target).backward()
            opt.step(slot.radii)
            dens.update(slot, W, H)
        return step
    steps = {}
    for name, wf in (("no features (a)", False), (f"{cf}-channel feature loss (a)", True), ("no features (b)", False),
                     (f"{cf}-channel feature loss (b)", True)):
        steps[name] = lambda step=make_step(rast, FrameSlot(), wf): timed(step)
    res = interleaved(steps)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii) + DensityStats.update()"
               f" [+ L1 on a {cf}-channel feature map, torch.optim.Adam on the features]")
    med = {}
    for name in steps:
        m = stats(res[name])
        med[name] = m[0]
        out.append(f"  {name:<34s}{fmt(m)}")
    plain = 0.5 * (med["no features (a)"] + med["no features (b)"])
    with_f = 0.5 * (med[f"{cf}-channel feature loss (a)"] + med[f"{cf}-channel feature loss (b)"])
    out.append(f"  with the feature loss against without: {with_f - plain:+.3f} ms (the L1 loss and torch's Adam over N x {cf} included); equal "
               f"configurations differ by {abs(med['no features (a)'] - med['no features (b)']):.3f} ms")
    del feats, opt_f, f_target
    torch.cuda.empty_cache()

    # ---- 3. the default step against the parent commit's library ----
    out.append("the default step (no features) through this tree's library and the parent commit's")
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


def finish(out):
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
