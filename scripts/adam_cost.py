"""What the optimiser step costs on the bench scene (bench.py's own scene builder, 1920 x 1080, one GPU): torch.optim.Adam in
its three implementations and gsrast_amd.optim.GaussianAdam (gsr_adam_step) — dense, with the frame's radii, and as one
launch per array instead of one for all five — over the same five raw arrays with the same gradients (those of one
render() + backward() of the frame: exact zeros where the frame culled), each optimiser with moments of its own; then the
whole training step, render() + loss.backward() + step(), with torch's fastest variant and with GaussianAdam. Bytes: what
the algorithm needs (28 per float updated; 4 per Gaussian for the radii). Medians of device-event times, every
configuration after its own warm-up, configurations interleaved round by round.
Usage: python scripts/adam_cost.py [--reps N] [--splats N] [--out FILE]   (the table of profiles/adam_cost.txt)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
ROW_FLOATS = 3 + 1 + 3 + 4 + 48
STEP_BYTES = 28 * ROW_FLOATS              # p, g, m, v read; p, m, v written


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
    return (f"  {what:<46s}{ms:8.3f} ms   {nbytes / 1e9:.3f} GB needed = {rate / 1e12:.2f} TB/s"
            f" = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")


def line_bytes(radii, row_bytes):
    """The bytes of the whole 128-byte lines that the visible rows of an array of `row_bytes` per row touch (the array
    taken as line-aligned): what a row-sparse pass over it cannot avoid moving."""
    rows = torch.nonzero(radii > 0).reshape(-1)
    first, last = rows * row_bytes // 128, (rows * row_bytes + row_bytes - 1) // 128
    touched = torch.zeros(int(radii.numel()) * row_bytes // 128 + 2, dtype=torch.bool, device=radii.device)
    for k in range((row_bytes + 126) // 128 + 1):           # (a row of 192 bytes lies in two or three lines)
        touched[torch.minimum(first + k, last)] = True
    return 128 * int(touched.sum())


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    make = lambda: GaussianParams.from_raw(*raw, device=dev)
    params = make()
    n = params.num_gaussians
    out = [f"adam cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds", f"bench frame ({label})"]

    # ---- the frame's gradients and radii ----
    rast = SplatRasterizer(W, H, device="cuda:0")
    dl = torch.randn((3, H, W), generator=torch.Generator().manual_seed(7)).to(dev)
    slot = RadiiSlot()
    (dl * render(params, rast, cam, radii_slot=slot)[0]).sum().backward()
    radii = slot.radii
    vis = int((radii > 0).sum())
    grads = [p.grad for p in params.parameters()]
    out.append(f"N = {n}, visible {vis} ({100 * vis / n:.0f} %), R = {rast.last_num_rendered}, plan {rast.last_plan}")
    out.append(f"a Gaussian is {ROW_FLOATS} raw floats; a step needs 28 B per float = {STEP_BYTES} B per Gaussian updated")

    # ---- the optimisers alone: the same values and gradients, moments of their own ----
    def clones():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in params.parameters()]
        for p, g in zip(ps, grads):
            p.grad = g
        return ps

    steps, refused = {}, {}
    for name, kw in (("default", {}), ("foreach=False", dict(foreach=False)), ("fused=True", dict(fused=True))):
        try:
            opt = torch.optim.Adam(clones(), lr=1e-4, eps=1e-15, **kw)
            opt.step()
            torch.cuda.synchronize()
            steps["torch " + name] = opt.step
        except Exception as e:                              # (a torch build without the fused kernel says so here)
            refused[name] = f"{type(e).__name__}: {str(e).splitlines()[0][:120]}"
    ours_dense = GaussianAdam(clones(), lr=1e-4, eps=1e-15)
    ours_sparse = GaussianAdam(clones(), lr=1e-4, eps=1e-15)
    steps["ours dense"] = ours_dense.step
    steps["ours radii"] = lambda: ours_sparse.step(radii)
    # one launch per array: an optimiser per array
    singles_dense = [GaussianAdam([p], lr=1e-4, eps=1e-15) for p in clones()]
    singles_sparse = [GaussianAdam([p], lr=1e-4, eps=1e-15) for p in clones()]
    steps["ours dense, a launch per array"] = lambda: [o.step() for o in singles_dense]
    steps["ours radii, a launch per array"] = lambda: [o.step(radii) for o in singles_sparse]

    for _ in range(3):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in steps}
    for _ in range(REPS):
        for k, fn in steps.items():
            ms[k].append(timed(fn))
    m = {k: float(np.median(v)) for k, v in ms.items()}
    torch_rows = {k: v for k, v in m.items() if k.startswith("torch ")}
    fastest = min(torch_rows, key=torch_rows.get)
    dense_bytes, sparse_bytes = STEP_BYTES * n, 4 * n + STEP_BYTES * vis
    out.append("the step alone, five arrays (bytes: what the algorithm needs)")
    for name in ("default", "foreach=False", "fused=True"):
        k = "torch " + name
        what = f"torch.optim.Adam, {name}"
        out.append(rate_line(what, m[k], dense_bytes) if k in m else f"  {what:<46s}refused by this torch build: {refused[name]}")
    out.append(rate_line("GaussianAdam, dense", m["ours dense"], dense_bytes))
    out.append(rate_line("GaussianAdam, the frame's radii", m["ours radii"], sparse_bytes))
    out.append(rate_line("  dense, one launch per array", m["ours dense, a launch per array"], dense_bytes))
    out.append(rate_line("  radii, one launch per array", m["ours radii, a launch per array"], sparse_bytes))
    lines = sum(line_bytes(radii, 4 * w) for w in (3, 1, 3, 4, 48))
    out.append(f"  whole 128-byte lines the visible rows touch: {100 * lines / (4 * ROW_FLOATS * n):.0f} % of the arrays "
               f"({7 * lines / 1e9:.3f} GB for the seven passes = {7 * lines / (m['ours radii'] * 1e-3) / 1e12:.2f} TB/s)")
    out.append(f"  torch's fastest is {fastest[6:]}: GaussianAdam dense takes {m['ours dense'] / m[fastest]:.2f} x its time, with radii "
               f"{m['ours radii'] / m[fastest]:.2f} x; radii / dense = {m['ours radii'] / m['ours dense']:.2f} (visible share {vis / n:.2f})")
    del steps, ours_dense, ours_sparse, singles_dense, singles_sparse
    torch.cuda.empty_cache()

    # ---- the whole step: render + backward + step (a rate of 1e-6: the frame stays the frame) ----
    kw = {"default": {}, "foreach=False": dict(foreach=False), "fused=True": dict(fused=True)}[fastest[6:]]
    p_torch, p_ours = make(), make()
    o_torch = torch.optim.Adam(p_torch.parameters(), lr=1e-6, eps=1e-15, **kw)
    o_ours = GaussianAdam(p_ours.parameters(), lr=1e-6, eps=1e-15)
    r_torch, r_ours = rast, SplatRasterizer(W, H, device="cuda:0")
    s_ours = RadiiSlot()

    def whole_torch():
        o_torch.zero_grad(set_to_none=True)
        (dl * render(p_torch, r_torch, cam)[0]).sum().backward()
        o_torch.step()

    def whole_ours():
        o_ours.zero_grad(set_to_none=True)
        (dl * render(p_ours, r_ours, cam, radii_slot=s_ours)[0]).sum().backward()
        o_ours.step(s_ours.radii)

    def no_step():
        for p in params.parameters():
            p.grad = None
        (dl * render(params, rast, cam)[0]).sum().backward()

    whole = {"none": no_step, "torch": whole_torch, "ours": whole_ours}
    for _ in range(3):
        for fn in whole.values():
            fn()
    torch.cuda.synchronize()
    wms = {k: [] for k in whole}
    for _ in range(REPS):
        for k, fn in whole.items():
            wms[k].append(timed(fn))
    wm = {k: float(np.median(v)) for k, v in wms.items()}
    out.append("one training step, colour loss")
    out.append(f"  render() + loss.backward(), no step                 {wm['none']:8.3f} ms")
    out.append(f"  ... + torch.optim.Adam ({fastest[6:]}).step()".ljust(54) + f"{wm['torch']:8.3f} ms ({wm['torch'] - wm['none']:+.3f} ms)")
    out.append(f"  ... + GaussianAdam.step(radii)".ljust(54) + f"{wm['ours']:8.3f} ms ({wm['ours'] - wm['none']:+.3f} ms)")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
