"""What the antialiased mode costs (gsr_antialias_forward / _backward, include/gsrast_amd_antialias.h) on the bench frame,
1920 x 1080, one GPU. Measured as scripts/alpha_grad_cost.py measures: medians of REPS rounds after warm-up, every round runs
every configuration once, in an order that rotates with the round.
  1. the two calls alone through the C entry points, device events around each call, with the bytes they move and what that
     is per second — beside gsr_mcmc_noise (68 bytes per row) in the same rounds, the streaming kernel they are held against:
       forward    48 B of rows + 4 B opacity in, o' and c out: 60 B per Gaussian (56 B with o' alone, as a trainer calls it)
       backward   every row live (radii NULL, no g zero): 4 B g + 48 B + 4 B in, 4 + 48 B out: 108 B (112 B with radii)
                  and as a training step calls it: the frame's radii and its dL/do' (most rows end after 8 bytes)
  2. the training step of INTEGRATION.md 2a — render() + photometric_loss + backward() + GaussianAdam.step(radii) — with and
     without antialiased=True, each entered twice (what two equal configurations differ by).
Usage: python scripts/antialias_cost.py [--reps N] [--splats N] [--out FILE]   (profiles/antialias_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd import autograd  # noqa: E402
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


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    out = [f"antialiased mode cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    params, rast, slot = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
    n = params.num_gaussians
    view, proj, cam_pos, tan_x, tan_y = autograd._camera_tensors(cam, dev)
    gen = torch.Generator().manual_seed(7)

    # ---- one antialiased step by hand: the activated arrays, the frame's radii and its dL/do' ----
    with torch.no_grad():
        frame = render(params, rast, cam, antialiased=True)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    with torch.no_grad():
        means3D, scales, rotations, opacities = (t.clone() for t in params.activated())
    o_leaf = autograd._antialias.compensation(means3D, scales, rotations, opacities, view, (tan_x, tan_y), W, H, proj=proj)[0].requires_grad_(True)
    color = autograd.rasterize(rast, means3D, scales, rotations, o_leaf, params.shs.detach(), view, proj, cam_pos, (tan_x, tan_y), radii_slot=slot)[0]
    photometric_loss(color, target).backward()
    g_frame, radii = o_leaf.grad.contiguous(), slot.radii
    out.append(f"N = {n}, R = {rast.last_num_rendered}, plan {rast.last_plan}; radii > 0: {int((radii > 0).sum())}, "
               f"dL/do' != 0: {int((g_frame != 0).sum())}")

    # ---- the two calls alone, and gsr_mcmc_noise beside them ----
    L = _capi.lib()
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    g_all = torch.randn((n,), generator=gen).to(dev).abs_().add_(0.1)

    def args(cls):
        a = cls()
        a.struct_size = C.sizeof(cls)
        a.num_gaussians, a.width, a.height = n, W, H
        a.tan_fovx, a.tan_fovy, a.scale_modifier = tan_x, tan_y, 1.0
        a.means3D, a.scales, a.rotations, a.opacities = means3D.data_ptr(), scales.data_ptr(), rotations.data_ptr(), opacities.data_ptr()
        a.view_matrix, a.proj_matrix, a.stream = view.data_ptr(), proj.data_ptr(), _capi.stream(dev)
        return a
    o_out, c_out, d_o, d_m, d_s, d_q = new(n), new(n), new(n), new(n, 4), new(n, 4), new(n, 4)
    f_both, f_one = args(_capi.AntialiasArgs), args(_capi.AntialiasArgs)
    f_both.opacities_out, f_both.compensation = o_out.data_ptr(), c_out.data_ptr()
    f_one.opacities_out = o_out.data_ptr()
    b_all, b_step = args(_capi.AntialiasBackwardArgs), args(_capi.AntialiasBackwardArgs)
    for b in (b_all, b_step):
        b.dL_dopacities, b.dL_dmeans3D, b.dL_dscales, b.dL_drotations = d_o.data_ptr(), d_m.data_ptr(), d_s.data_ptr(), d_q.data_ptr()
    b_all.dL_dopacities_out = g_all.data_ptr()
    b_step.dL_dopacities_out, b_step.radii = g_frame.data_ptr(), radii.data_ptr()
    noise = _capi.McmcNoiseArgs()
    noise.struct_size, noise.scaler, noise.n = C.sizeof(_capi.McmcNoiseArgs), 0.0, n          # (scaler 0: xyz keeps its bits)
    xyz, eps = params.xyz.detach().clone(), torch.randn((n, 3), generator=gen).to(dev)
    noise.xyz, noise.opacity_logit, noise.log_scale = xyz.data_ptr(), params.opacity_logit.data_ptr(), params.log_scale.data_ptr()
    noise.rotation, noise.noise, noise.stream = params.rotation.data_ptr(), eps.data_ptr(), _capi.stream(dev)
    live = int(((radii > 0) & (g_frame != 0)).sum())
    calls = {"gsr_mcmc_noise": (L.gsr_mcmc_noise, noise, 68 * n),
             "gsr_antialias_forward, o' and c": (L.gsr_antialias_forward, f_both, 60 * n),
             "gsr_antialias_forward, o' alone": (L.gsr_antialias_forward, f_one, 56 * n),
             "gsr_antialias_backward, every row live": (L.gsr_antialias_backward, b_all, 108 * n),
             "gsr_antialias_backward, the step's radii and g": (L.gsr_antialias_backward, b_step, (4 + 4 + 52) * n + 52 * live),
             }
    with torch.cuda.device(dev):
        got = interleaved({k: (lambda fn=fn, a=a, k=k: timed(lambda: _capi.check(fn(C.byref(a)), k))) for k, (fn, a, _) in calls.items()})
    out.append("the calls alone (device events around the call; bytes: what the call must move)")
    rate = {}
    for k, (_, _, nbytes) in calls.items():
        m = stats(got[k])
        rate[k] = nbytes / (m[0] * 1e-3)
        out.append(f"  {k:<48s}{m[0]:7.4f} ms ({m[1]:.4f} .. {m[2]:.4f})   {nbytes / 1e9:.3f} GB   {rate[k] / 1e12:.2f} TB/s = "
                   f"{100.0 * rate[k] / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak")
    for k in list(calls)[1:4]:
        out.append(f"  {k}: {rate[k] / rate['gsr_mcmc_noise']:.2f} of gsr_mcmc_noise's bandwidth in the same rounds")

    # ---- the training step of INTEGRATION.md 2a ----
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    steps = {}
    for name, aa in (("as it is (a)", False), ("antialiased=True (a)", True), ("as it is (b)", False), ("antialiased=True (b)", True)):
        def step(aa=aa):
            opt.zero_grad(set_to_none=True)
            color, _, _ = render(params, rast, cam, radii_slot=slot, antialiased=aa)
            photometric_loss(color, target).backward()
            opt.step(slot.radii)
        steps[name] = lambda step=step: timed(step)
    got = interleaved(steps, warm=3)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii)")
    med = {}
    for name in steps:
        m = stats(got[name])
        med[name] = m[0]
        out.append(f"  {name:<28s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
    plain = 0.5 * (med["as it is (a)"] + med["as it is (b)"])
    anti = 0.5 * (med["antialiased=True (a)"] + med["antialiased=True (b)"])
    out.append(f"  antialiased against the default: {anti - plain:+.3f} ms; equal configurations differ by "
               f"{abs(med['as it is (a)'] - med['as it is (b)']):.3f} / {abs(med['antialiased=True (a)'] - med['antialiased=True (b)']):.3f} ms")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
