"""What the camera gradients cost: the camera pass alone (gsr_camera_backward: device events around its two kernels, and the
bytes it must move over that time), and forward + backward with and without camera=True, on the bench frame, the far pose
(0, 0, -30) and the trained-like scene. 1920 x 1080, one GPU, a depth gradient in every backward; medians of device-event
times, each configuration after its own warm-up, configurations interleaved round by round so that clock drift spreads over
all of them.
Usage: python scripts/camera_grad_cost.py [--reps N] [--out FILE]   (the table of profiles/camera_grad_cost.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import camera, scenes  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
HBM_PEAK = 8.0e12      # MI355X HBM3E, bytes/s (spec)


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def frame_table(title, scene, near, far, pos):
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(scene)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    gd = torch.randn((H, W), generator=torch.Generator().manual_seed(3)).cuda()
    dl = torch.randn((3, H, W), generator=torch.Generator().manual_seed(7)).cuda()
    for cam_on in (False, True):                     # warm-up (the tile history settles)
        for _ in range(3):
            r.draw(cam)
            r.backward(dl, dL_ddepth=gd, camera=cam_on)
    r.draw(cam)
    grads = {k: v.clone() for k, v in r.backward(dl, dL_ddepth=gd).items()}
    n = r.num_gaussians
    vis = int((r.map_geometry_state()["radii"] > 0).sum())
    # radii for all; means3D 16, cov3D 24, dL_dmean2D 8, dL_dcov2D 16, dL_ddepths 4 per visible Gaussian (whole lines
    # are fetched: the figure is what the pass needs, not what the memory moves)
    nbytes = 4 * n + 68 * vis
    for _ in range(5):
        r.camera_backward(grads, depth=True)
    pass_ms, fb = [], {False: [], True: []}
    for _ in range(REPS):
        r.camera_backward(grads, depth=True, profile=True)
        pass_ms.append(r.last_camera_ms)
        for cam_on in (False, True):
            fb[cam_on].append(timed(lambda: (r.draw(cam, sync=False), r.backward(dl, dL_ddepth=gd, camera=cam_on))))
    t = float(np.median(pass_ms))
    base, with_cam = float(np.median(fb[False])), float(np.median(fb[True]))
    rate = nbytes / (t * 1e-3)
    lines = [f"{title}: N = {n}, visible {vis} ({100 * vis / n:.0f} %), R = {r.last_num_rendered}, plan {r.last_plan}",
             f"  camera pass alone                  {1e3 * t:7.1f} us   {nbytes / 1e9:.3f} GB needed = {rate / 1e12:.2f} TB/s"
             f" = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak",
             f"  forward + backward                 {base:7.3f} ms",
             f"  forward + backward, camera=True    {with_cam:7.3f} ms ({100 * (with_cam / base - 1):+5.1f} %)"]
    print("\n".join(lines), flush=True)
    return lines


def main():
    dev = torch.device("cuda:0")
    out = [f"camera gradient cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds, depth gradient on"]
    sc, near, far, pos, label = bench.make_scene("garden_like", bench.DEFAULT_SPLATS, dev)
    out += frame_table(f"bench frame ({label})", sc, near, far, pos)
    out += frame_table("far pose (0, 0, -30)", sc, near, far, (0.0, 0.0, -30.0))
    del sc
    torch.cuda.empty_cache()
    tl = scenes.trained_like(bench.DEFAULT_SPLATS, seed=45)
    out += frame_table("trained-like scene (0, 0, -14)", tl, near, far, (0.0, 0.0, -14.0))
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
