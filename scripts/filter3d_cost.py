"""What the 3D smoothing filter costs (gsr_filter3d_*, include/gsrast_amd_filter3d.h) on the bench scene, 1920 x 1080, one GPU.
Measured as scripts/antialias_cost.py measures: medians of REPS rounds after warm-up, every round runs every configuration
once, in an order that rotates with the round. One set of cameras: the bench's camera path (bench.walk_path).
  1. Filter3D.compute over those cameras against a torch transcription of upstream's compute_3D_filter on the same device
     (float32, upstream's ops in upstream's order: about fifteen launches per camera over all N Gaussians).
  2. the smoothing alone through the C entry points, device events around each call, with the bytes they move:
       forward    16 B scales + 4 B opacity + 4 B filter in, 16 + 4 B out: 44 B per Gaussian
       backward   every row live (radii NULL): 24 B + 16 + 4 B gradients in, 16 + 4 B out: 64 B (68 B with radii)
                  and as a training step calls it: the frame's radii and gradients (a culled row ends after 4 bytes)
  3. the training step of INTEGRATION.md 2a — render() + photometric_loss + backward() + GaussianAdam.step(radii) — with
     antialiased=True, with and without filter_3d, each entered twice (what two equal configurations differ by).
  4. the step with filter_3d=None (and antialiased=False) through this tree's library against the same step through the
     parent commit's library — built from a checkout of that commit (python -m gsrast_amd.build --tag parent there) and named
     with --parent-lib; loaded beside this tree's into the same process, the two interleaved. The difference is held against
     the parent's own inter-quartile spread. Without --parent-lib the row says "not measured".
Usage: python scripts/filter3d_cost.py [--reps N] [--splats N] [--cameras N] [--parent-lib PATH] [--out FILE]   (profiles/filter3d_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera, filter3d  # noqa: E402
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
CAMERAS = _arg("--cameras", 120)
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


def upstream_compute_3d_filter(xyz, cams):
    """Upstream's compute_3D_filter (Mip-Splatting, scene/gaussian_model.py), op for op, on xyz's device in float32.
    cams: (R [3,3], T [3], focal_x, focal_y, width, height), R and T device tensors with xyz_cam = xyz @ R + T."""
    distance = torch.ones((xyz.shape[0]), device=xyz.device) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), device=xyz.device, dtype=torch.bool)
    focal_length = 0.0
    for R, T, focal_x, focal_y, width, height in cams:
        xyz_cam = xyz @ R + T[None, :]
        xyz_to_cam = torch.norm(xyz_cam, dim=1)          # noqa: F841 (upstream computes it and does not use it)
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z = torch.clamp(z, min=0.001)
        x = x / z * focal_x + width / 2.0
        y = y / z * focal_y + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < focal_x:
            focal_length = focal_x
    distance[~valid_points] = distance[valid_points].max()
    return distance / focal_length * (0.2 ** 0.5)


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point it has gets this tree's signature."""
    P = C.CDLL(os.path.abspath(path))
    tables = (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
              _capi.ANTIALIAS_SIGNATURES)
    for table in tables:
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_filter3d_forward"), "--parent-lib exports gsr_filter3d_forward: it is not the parent commit's"
    return P


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    cams = bench.walk_path(W, H, near, far, frames=CAMERAS)
    out = [f"3D smoothing filter cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench scene ({label}); {len(cams)} cameras of the bench's camera path"]
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    this_lib = _capi.lib()
    params, rast, slot = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
    n = params.num_gaussians
    gen = torch.Generator().manual_seed(7)

    # ---- 1. compute against upstream's loop ----
    f3 = filter3d.Filter3D(n, dev)
    xyz = params.xyz.detach()
    up_cams = []
    for c in cams:
        V = np.asarray(c.view, np.float32).reshape(4, 4).T
        up_cams.append((torch.from_numpy(V[:3, :3].T.copy()).to(dev), torch.from_numpy(V[:3, 3].copy()).to(dev),
                        float(np.float32(c.width) / (np.float32(2.0) * np.float32(c.tan_fovx))),
                        float(np.float32(c.height) / (np.float32(2.0) * np.float32(c.tan_fovy))), c.width, c.height))
    records, max_focal = filter3d.camera_records(cams)
    rec_dev = torch.from_numpy(records).to(dev)

    def kernels_alone():
        f3.reset()
        a = _capi.Filter3dObserveArgs()
        a.struct_size, a.flags, a.num_gaussians, a.position_stride, a.num_cameras = C.sizeof(a), 0, n, 3, len(cams)
        a.positions, a.cameras, a.min_depth, a.stream = xyz.data_ptr(), rec_dev.data_ptr(), f3.min_depth.data_ptr(), _capi.stream(dev)
        _capi.call("gsr_filter3d_observe", C.byref(a), device=dev)
        f3.max_focal = max_focal
        f3.finalize()
    with torch.no_grad():
        mine, theirs = f3.compute(params, cams), upstream_compute_3d_filter(xyz, up_cams)
        seen = int((f3.min_depth < float("inf")).sum())
        rel = (mine - theirs).abs() / theirs
        apart, rel = int((rel > 1e-5).sum()), float(rel.max())
        got = interleaved({"Filter3D.compute (records made and uploaded, reset, observe, finalize)": lambda: timed(lambda: f3.compute(params, cams)),
                           "  of which reset + gsr_filter3d_observe + gsr_filter3d_finalize": lambda: timed(kernels_alone),
                           "upstream's loop in torch (float32, same device)": lambda: timed(lambda: upstream_compute_3d_filter(xyz, up_cams))},
                          reps=max(4, REPS // 4), warm=2)
    out.append(f"N = {n}; seen by a camera: {seen}; the two filters differ by more than 1e-5 relative in {apart} rows, at most by {rel:.2e} "
               "(both in float32; torch's matrix product rounds t in another order, so a pair on a boundary can be decided the other way and another camera be the nearest)")
    out.append("compute_3D_filter (device events around the whole call, host work included)")
    med = {}
    for k, v in got.items():
        m = stats(v)
        med[k] = m[0]
        out.append(f"  {k:<76s}{m[0]:9.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
    keys = list(got)
    pairs = n * len(cams)
    out.append(f"  upstream's loop / Filter3D.compute: {med[keys[2]] / med[keys[0]]:.1f} x; the kernels: {pairs / (med[keys[1]] * 1e-3) / 1e9:.1f} G pairs/s")
    filt = f3.values

    # ---- 2. the smoothing alone ----
    with torch.no_grad():
        _, scales, _, opacities = (t.clone() for t in params.activated())
        frame = render(params, rast, cam, antialiased=True, filter_3d=filt)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    opt.zero_grad(set_to_none=True)
    photometric_loss(render(params, rast, cam, radii_slot=slot, antialiased=True, filter_3d=filt)[0], target).backward()
    radii = slot.radii
    visible = int((radii > 0).sum())
    out.append(f"R = {rast.last_num_rendered}, plan {rast.last_plan}; radii > 0: {visible}")
    L = this_lib
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    g_s, g_o = torch.randn((n, 4), generator=gen).to(dev), torch.randn((n,), generator=gen).to(dev)
    s_out, o_out, d_s, d_o = new(n, 4), new(n), new(n, 4), new(n)
    fwd = _capi.Filter3dArgs()
    fwd.struct_size, fwd.flags, fwd.num_gaussians = C.sizeof(fwd), 0, n
    fwd.scales, fwd.opacities, fwd.filter = scales.data_ptr(), opacities.data_ptr(), filt.data_ptr()
    fwd.scales_out, fwd.opacities_out, fwd.stream = s_out.data_ptr(), o_out.data_ptr(), _capi.stream(dev)

    def backward_args(with_radii):
        b = _capi.Filter3dBackwardArgs()
        b.struct_size, b.flags, b.num_gaussians = C.sizeof(b), 0, n
        b.scales, b.opacities, b.filter = scales.data_ptr(), opacities.data_ptr(), filt.data_ptr()
        b.dL_dscales_out, b.dL_dopacities_out = g_s.data_ptr(), g_o.data_ptr()
        b.radii = radii.data_ptr() if with_radii else None
        b.dL_dscales, b.dL_dopacities, b.stream = d_s.data_ptr(), d_o.data_ptr(), _capi.stream(dev)
        return b
    calls = {"gsr_filter3d_forward": (L.gsr_filter3d_forward, fwd, 44 * n),
             "gsr_filter3d_backward, every row live": (L.gsr_filter3d_backward, backward_args(False), 64 * n),
             "gsr_filter3d_backward, the step's radii": (L.gsr_filter3d_backward, backward_args(True), (4 + 20) * n + 44 * visible)}
    with torch.cuda.device(dev):
        got = interleaved({k: (lambda fn=fn, a=a, k=k: timed(lambda: _capi.check(fn(C.byref(a)), k))) for k, (fn, a, _) in calls.items()})
    out.append("the smoothing alone (device events around the call; bytes: what the call must move)")
    for k, (_, _, nbytes) in calls.items():
        m = stats(got[k])
        rate = nbytes / (m[0] * 1e-3)
        out.append(f"  {k:<44s}{m[0]:7.4f} ms ({m[1]:.4f} .. {m[2]:.4f})   {nbytes / 1e9:.3f} GB   {rate / 1e12:.2f} TB/s = "
                   f"{100.0 * rate / HBM_PEAK:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s peak")

    # ---- 3. the training step of INTEGRATION.md 2a, antialiased, with and without the filter ----
    def make_step(r, s, **kw):
        def step():
            opt.zero_grad(set_to_none=True)
            color, _, _ = render(params, r, cam, radii_slot=s, **kw)
            photometric_loss(color, target).backward()
            opt.step(s.radii)
        return step
    steps = {}
    for name, kw in (("antialiased (a)", {}), ("antialiased, filter_3d (a)", {"filter_3d": filt}), ("antialiased (b)", {}),
                     ("antialiased, filter_3d (b)", {"filter_3d": filt})):
        steps[name] = lambda step=make_step(rast, slot, antialiased=True, **kw): timed(step)
    got = interleaved(steps, warm=3)
    out.append("one training step: render(antialiased=True) + photometric_loss + backward() + GaussianAdam.step(radii)")
    med = {}
    for name in steps:
        m = stats(got[name])
        med[name] = m[0]
        out.append(f"  {name:<32s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
    plain = 0.5 * (med["antialiased (a)"] + med["antialiased (b)"])
    filtered = 0.5 * (med["antialiased, filter_3d (a)"] + med["antialiased, filter_3d (b)"])
    out.append(f"  with filter_3d against without: {filtered - plain:+.3f} ms; equal configurations differ by "
               f"{abs(med['antialiased (a)'] - med['antialiased (b)']):.3f} / "
               f"{abs(med['antialiased, filter_3d (a)'] - med['antialiased, filter_3d (b)']):.3f} ms")

    # ---- 4. filter_3d=None against the parent commit's library ----
    out.append("the default step, render() + photometric_loss + backward() + GaussianAdam.step(radii), filter_3d=None")
    if PARENT:
        P = load_parent(PARENT)

        def through(lib):
            """A step whose every call goes through `lib`: a rasterizer made under it, and the ctypes table pointed at it."""
            _capi._lib = lib
            r, s = SplatRasterizer(W, H, device="cuda:0"), RadiiSlot()
            inner = make_step(r, s)

            def step():
                _capi._lib = lib
                inner()
            return step
        steps = {"parent commit (a)": through(P), "this tree (a)": through(this_lib), "parent commit (b)": through(P), "this tree (b)": through(this_lib)}
        got = interleaved({k: (lambda fn=fn: timed(fn)) for k, fn in steps.items()}, warm=3)
        _capi._lib = this_lib
        med, quart = {}, {}
        for name in steps:
            m = stats(got[name])
            med[name], quart[name] = m[0], (m[1], m[2])
            out.append(f"  {name:<32s}{m[0]:8.3f} ms ({m[1]:.3f} .. {m[2]:.3f})")
        parent = 0.5 * (med["parent commit (a)"] + med["parent commit (b)"])
        mine = 0.5 * (med["this tree (a)"] + med["this tree (b)"])
        lo = min(quart["parent commit (a)"][0], quart["parent commit (b)"][0])
        hi = max(quart["parent commit (a)"][1], quart["parent commit (b)"][1])
        inside = lo <= mine <= hi
        out.append(f"  this tree {mine:.3f} ms against the parent {parent:.3f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own quartiles "
                   f"{lo:.3f} .. {hi:.3f} ms ({1e3 * (hi - lo):.1f} us): {'inside' if inside else 'OUTSIDE'}")
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
