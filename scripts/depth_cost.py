"""What the depth channel costs: draw() with and without depth (both modes) on the bench frame, the far pose and the trained-like
scene, and forward + backward with dL_ddepth. 1920 x 1080, one GPU; medians of CUDA-event times over the repeats, each
configuration after its own warm-up, configurations interleaved round by round so that clock drift spreads over all of them.
Blend kernel time from the library's own stage events (GSR_FLAG_PROFILE).
Usage: python scripts/depth_cost.py [--reps N] [--out FILE]   (the table of profiles/depth_cost.txt)"""
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
    modes = {"no depth": False, "depth": True, "inverse depth": "inverse"}
    total = {k: [] for k in modes}
    blend = {k: [] for k in modes}
    for k, m in modes.items():                       # warm-up (the tile history settles)
        for _ in range(5):
            r.draw(cam, depth=m)
    for _ in range(REPS):
        for k, m in modes.items():
            total[k].append(timed(lambda: r.draw(cam, depth=m, sync=False)))
            r.draw(cam, depth=m, profile=True)
            blend[k].append(r.last_stage_ms["blend"])
    lines = [f"{title}: R = {r.last_num_rendered}, plan {r.last_plan}, deep tiles {r.last_deep_tiles}"]
    base_t, base_b = np.median(total["no depth"]), np.median(blend["no depth"])
    for k in modes:
        t, b = np.median(total[k]), np.median(blend[k])
        lines.append(f"  draw {k:14s} {t:7.3f} ms ({100 * (t / base_t - 1):+5.1f} %)   blend {b:6.3f} ms ({100 * (b / base_b - 1):+5.1f} %)")
    fb = {"colour only": None, "with dL_ddepth": gd}
    res = {}
    for k, g in fb.items():
        for _ in range(3):
            r.draw(cam, depth=g is not None)
            r.backward(dl, dL_ddepth=g)
        ts = []
        for _ in range(max(5, REPS // 3)):
            ts.append(timed(lambda: (r.draw(cam, depth=g is not None, sync=False), r.backward(dl, dL_ddepth=g))))
        res[k] = float(np.median(ts))
    base = res["colour only"]
    for k, t in res.items():
        lines.append(f"  forward + backward, {k:14s} {t:7.3f} ms ({100 * (t / base - 1):+5.1f} %)")
    print("\n".join(lines), flush=True)
    return lines


def main():
    dev = torch.device("cuda:0")
    out = [f"depth channel cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} draws"]
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
