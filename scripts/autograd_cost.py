"""What the autograd layer costs on the bench scene (bench.py's own scene builder, 1920 x 1080, one GPU): the device time of
the two activation kernels (gsr_activate_params / _backward) and the bytes/s they reach against the bytes the algorithm
needs; the same activations, forward and backward, written in torch ops; and one full training step through
`render(...)` + `loss.backward()` against the same frame done by hand with draw() + backward(). Medians of device-event
times, every configuration after its own warm-up, configurations interleaved round by round.
Usage: python scripts/autograd_cost.py [--reps N] [--splats N] [--out FILE]   (the table of profiles/autograd_cost.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, activate, render  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080


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


def rate_line(what, ms, nbytes):
    rate = nbytes / (ms * 1e-3)
    return (f"  {what:<46s}{1e3 * ms:8.1f} us   {nbytes / 1e9:.3f} GB needed = {rate / 1e12:.2f} TB/s"
            f" = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")


def torch_activations(xyz, x, s, r):
    one = torch.ones_like(xyz[:, :1])
    return (torch.cat([xyz, one], 1), torch.cat([torch.exp(s), one * float(np.e)], 1),
            r / torch.sqrt((r * r).sum(1, keepdim=True)), torch.sigmoid(x))


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    params = GaussianParams.from_raw(sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)),
                                     sc["rotations"], sc["shs"], device=dev)
    n = params.num_gaussians
    out = [f"autograd cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds", f"bench frame ({label})"]

    # ---- the frame by hand: the activated arrays as a static scene ----
    with torch.no_grad():
        act = params.activated()
    hand = SplatRasterizer(W, H, device="cuda:0")
    hand.bind_scene(*act, params.shs.detach())
    dl = torch.randn((3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
    for _ in range(3):
        hand.draw(cam)
        hand.backward(dl)
    hand.draw(cam)
    grads = {k: v.clone() for k, v in hand.backward(dl).items()}
    radii = hand.map_geometry_state()["radii"].clone()
    vis = int((radii > 0).sum())
    out.append(f"N = {n}, visible {vis} ({100 * vis / n:.0f} %), R = {hand.last_num_rendered}, plan {hand.last_plan}")

    # ---- the two kernels alone ----
    L = _capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    d_xyz, d_op, d_scale, d_rot = new(n, 3), new(n), new(n, 3), new(n, 4)

    def kernel_backward(rad):
        _capi.check(L.gsr_activate_params_backward(
            n, params.opacity_logit.data_ptr(), params.log_scale.data_ptr(), params.rotation.data_ptr(),
            rad.data_ptr() if rad is not None else None, grads["dL_dmeans3D"].data_ptr(), grads["dL_dscales"].data_ptr(),
            grads["dL_drotations"].data_ptr(), grads["dL_dconic_opacity"].data_ptr(), d_xyz.data_ptr(), d_op.data_ptr(),
            d_scale.data_ptr(), d_rot.data_ptr(), stream), "gsr_activate_params_backward")

    def kernel_forward():
        with torch.no_grad():
            activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)

    # ---- the same in torch ops ----
    leaves = [p.detach().clone().requires_grad_(True) for p in (params.xyz, params.opacity_logit, params.log_scale, params.rotation)]
    gouts = (grads["dL_dmeans3D"], grads["dL_dscales"], grads["dL_drotations"], grads["dL_dconic_opacity"][:, 3].contiguous())
    held = {}

    def torch_forward():
        held["out"] = torch_activations(*leaves)

    def torch_backward():
        torch.autograd.backward(held["out"], gouts)
        for t in leaves:
            t.grad = None

    # ---- one full step ----
    rast = SplatRasterizer(W, H, device="cuda:0")

    def step_autograd():
        color, _, _ = render(params, rast, cam)
        (dl * color).sum().backward()
        for p in params.parameters():
            p.grad = None

    def step_by_hand():
        hand.draw(cam, sync=False)
        hand.backward(dl)

    def step_by_hand_subset():
        hand.draw(cam, sync=False)
        hand.backward(dl, outputs=("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dconic_opacity", "dL_dshs"))

    for _ in range(3):                                    # warm-up of every configuration
        kernel_forward(), kernel_backward(None), kernel_backward(radii), torch_forward(), torch_backward()
        step_autograd(), step_by_hand(), step_by_hand_subset()
    torch.cuda.synchronize()
    names = ("fwd", "bwd", "bwd_radii", "t_fwd", "t_bwd", "step", "hand", "hand_subset")
    ms = {k: [] for k in names}
    for _ in range(REPS):
        ms["fwd"].append(timed(kernel_forward))
        ms["bwd"].append(timed(lambda: kernel_backward(None)))
        ms["bwd_radii"].append(timed(lambda: kernel_backward(radii)))
        ms["t_fwd"].append(timed(torch_forward))
        ms["t_bwd"].append(timed(torch_backward))
        ms["step"].append(timed(step_autograd))
        ms["hand"].append(timed(step_by_hand))
        ms["hand_subset"].append(timed(step_by_hand_subset))
    m = {k: float(np.median(v)) for k, v in ms.items()}
    out.append("activation kernels (bytes: what the algorithm needs per Gaussian; whole lines are fetched)")
    out.append(rate_line("gsr_activate_params (44 B read + 52 B written)", m["fwd"], 96 * n))
    out.append(rate_line("gsr_activate_params_backward (100 + 44 B)", m["bwd"], 144 * n))
    out.append(rate_line("  with radii (4 B, + 96 B if visible; + 44 B)", m["bwd_radii"], 48 * n + 96 * vis))
    out.append("the same activations in torch ops")
    out.append(f"  forward  {m['t_fwd']:8.3f} ms ({m['t_fwd'] / m['fwd']:.1f} x the kernel)")
    out.append(f"  backward {m['t_bwd']:8.3f} ms ({m['t_bwd'] / m['bwd_radii']:.1f} x the kernel with radii)")
    out.append("one step, forward + backward, colour loss")
    out.append(f"  draw() + backward() by hand, every output         {m['hand']:8.3f} ms")
    out.append(f"  draw() + backward() by hand, the trainer's five   {m['hand_subset']:8.3f} ms")
    out.append(f"  render() + loss.backward()                        {m['step']:8.3f} ms"
               f" ({m['step'] - m['hand_subset']:+.3f} ms: activations, fresh outputs, autograd)")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
