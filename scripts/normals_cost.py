"""What the two operators of the normal-consistency loss cost (gsr_gaussian_normals_forward / _backward, gsr_depth_normals_forward /
_backward, include/gsrast_amd_normals.h) on the bench frame, 1920 x 1080, one GPU. Four measurements, reported and not asserted:
  1. each of the four calls (the whole Python call by device events), on the frame's 5.83 M Gaussians and on its expected depth;
  2. the same operators composed of torch operations on the same device (`torch_gaussian_normals` and `torch_depth_normals` below,
     forward and forward + backward by autograd), and the ratio;
  3. the training step of INTEGRATION.md 2a with the normal-consistency term (depth, a differentiable opacity map and the normal
     map beside the photometric loss), and without;
  4. the default step (no normals) through this tree's library and through the parent commit's — built from a checkout of that
     commit (python -m gsrast_amd.build there) and named with --parent-lib; loaded beside this tree's into the same process, the
     two interleaved, as scripts/distortion_cost.py does. Without --parent-lib the row says "not measured".
Medians of REPS rounds after warm-up; every round runs every configuration once, in an order that rotates with the round.
Usage: python scripts/normals_cost.py [--reps N] [--splats N] [--parent-lib PATH] [--out FILE] [--only-passes]
(profiles/normals_cost.txt)"""
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
                  _capi.DISTORTION_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    assert not hasattr(P, "gsr_depth_normals_forward"), "--parent-lib exports gsr_depth_normals_forward: it is not the parent commit's"
    return P


def torch_gaussian_normals(means3D, scales, rotations, view):
    """gaussian_normals(semantics="gscuda") of torch operations: the rotation matrix of the normalised quaternion, its column of
    the smallest scale, the view matrix's 3 x 3 part, the flip towards the camera, the normalisation."""
    q = rotations / rotations.norm(dim=1, keepdim=True)
    x, y, z, w = q.unbind(1)
    Rm = torch.stack([2 * (x * x + y * y) - 1, 2 * (y * z - x * w), 2 * (y * w + x * z),
                      2 * (y * z + x * w), 2 * (x * x + z * z) - 1, 2 * (z * w - x * y),
                      2 * (y * w - x * z), 2 * (z * w + x * y), 2 * (x * x + w * w) - 1], 1).reshape(-1, 3, 3)
    a = scales[:, :3].argmin(1)
    nw = torch.gather(Rm, 2, a[:, None, None].expand(-1, 3, 1)).squeeze(2)
    V = view.reshape(4, 4).t()
    nv = nw @ V[:3, :3].t()
    t = means3D[:, :3] @ V[:3, :3].t() + V[:3, 3]
    nv = torch.where(((nv * t).sum(1) > 0)[:, None], -nv, nv)
    return nv / nv.norm(dim=1, keepdim=True)


def torch_depth_normals(depth, tan_fov):
    """depth_normals(semantics="gscuda") of torch operations: unproject, four shifted slices, cross product, normalise, pad."""
    h, w = depth.shape
    rx = (2.0 * torch.arange(w, device=depth.device, dtype=torch.float32) / w - 1.0) * tan_fov[0]
    ry = (2.0 * torch.arange(h, device=depth.device, dtype=torch.float32) / h - 1.0) * tan_fov[1]
    P = torch.stack([rx[None, :] * depth, ry[:, None] * depth, depth])
    dv = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    dh = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    c = torch.cross(dv, dh, dim=0)
    ok = ((depth[2:, 1:-1] > 0) & (depth[:-2, 1:-1] > 0) & (depth[1:-1, 2:] > 0) & (depth[1:-1, :-2] > 0))
    n = torch.where(ok, c / c.norm(dim=0, keepdim=True).clamp_min(1e-30), torch.zeros_like(c))
    return torch.nn.functional.pad(n, (1, 1, 1, 1))


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    tan = (float(cam.tan_fovx), float(cam.tan_fovy))
    out = [f"normal-consistency operators' cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians (and quartiles) of {REPS} interleaved rounds",
           f"bench frame ({label})"]
    this_lib = _capi.lib()
    gen = torch.Generator().manual_seed(7)

    # ---- 1, 2. the four calls beside their torch compositions ----
    r = SplatRasterizer(W, H, device="cuda:0")
    r.configure_from_scene(sc)
    n = r.num_gaussians
    for _ in range(5):                                    # (the tile history settles)
        r.draw(cam, depth=True)
    out.append(f"N = {n}, R = {r.last_num_rendered}, plan {r.last_plan}")
    view = torch.from_numpy(np.asarray(cam.view, np.float32).reshape(-1)).to(dev)
    into = {"out_color": torch.empty((3, H, W), device=dev), "out_depth": torch.empty((H, W), device=dev)}
    r.draw(cam, depth=True, into=into)
    depth = (into["out_depth"] / r.opacity_map().clamp_min(1e-6)).contiguous()
    m3, s3, q3 = r.means3D, r.scales, r.rotations
    g_n = torch.randn((n, 3), generator=gen).to(dev)
    g_d = torch.randn((3, H, W), generator=gen).to(dev)
    q_leaf = q3.clone().requires_grad_(True)
    d_leaf = depth.clone().requires_grad_(True)
    del r
    torch.cuda.empty_cache()

    def fwd_bwd(fn, leaf, g):
        def run():
            leaf.grad = None
            (fn() * g).sum().backward()
        return run
    fns = {"g_fwd": lambda: timed(lambda: normals.gaussian_normals(m3, s3, q3, view)),
           "g_both": lambda: timed(fwd_bwd(lambda: normals.gaussian_normals(m3, s3, q_leaf, view), q_leaf, g_n)),
           "g_fwd_torch": lambda: timed(lambda: torch_gaussian_normals(m3, s3, q3, view)),
           "g_both_torch": lambda: timed(fwd_bwd(lambda: torch_gaussian_normals(m3, s3, q_leaf, view), q_leaf, g_n)),
           "d_fwd": lambda: timed(lambda: normals.depth_normals(depth, tan)),
           "d_both": lambda: timed(fwd_bwd(lambda: normals.depth_normals(d_leaf, tan), d_leaf, g_d)),
           "d_fwd_torch": lambda: timed(lambda: torch_depth_normals(depth, tan)),
           "d_both_torch": lambda: timed(fwd_bwd(lambda: torch_depth_normals(d_leaf, tan), d_leaf, g_d))}
    # the backward calls alone: the autograd functions' own, on a graph kept from one forward
    kept_g = normals.gaussian_normals(m3, s3, q_leaf, view)
    kept_d = normals.depth_normals(d_leaf, tan)
    fns["g_bwd"] = lambda: timed(lambda: torch.autograd.grad(kept_g, q_leaf, g_n, retain_graph=True))
    fns["d_bwd"] = lambda: timed(lambda: torch.autograd.grad(kept_d, d_leaf, g_d, retain_graph=True))
    s = {k: stats(v) for k, v in interleaved(fns).items()}
    apart = (normals.gaussian_normals(m3, s3, q3, view) - torch_gaussian_normals(m3, s3, q3, view)).abs().nan_to_num(0.0).max(1).values
    close_d = float((normals.depth_normals(depth, tan) - torch_depth_normals(depth, tan)).abs().max())
    out.append(f"(the compositions compute the same functions: all but {int((apart > 1e-4).sum())} of {n} Gaussians within 1e-4 — rows whose flip "
               f"or shortest axis the other rounding decides otherwise — the rest within {float(apart[apart <= 1e-4].max()):.1e}; every pixel within {close_d:.1e})")
    out.append(f"the per-Gaussian normal, N = {n}")
    out.append(f"  gaussian_normals, forward                             {fmt(s['g_fwd'])}")
    out.append(f"  gaussian_normals, backward alone                      {fmt(s['g_bwd'])}")
    out.append(f"  gaussian_normals, forward + backward                  {fmt(s['g_both'])}")
    out.append(f"  the torch composition, forward                        {fmt(s['g_fwd_torch'])}   x {s['g_fwd_torch'][0] / s['g_fwd'][0]:.1f}")
    out.append(f"  the torch composition, forward + backward             {fmt(s['g_both_torch'])}   x {s['g_both_torch'][0] / s['g_both'][0]:.1f}")
    out.append(f"the depth normal, {W} x {H}")
    out.append(f"  depth_normals, forward                                {fmt(s['d_fwd'])}")
    out.append(f"  depth_normals, backward alone                         {fmt(s['d_bwd'])}")
    out.append(f"  depth_normals, forward + backward                     {fmt(s['d_both'])}")
    out.append(f"  the torch composition, forward                        {fmt(s['d_fwd_torch'])}   x {s['d_fwd_torch'][0] / s['d_fwd'][0]:.1f}")
    out.append(f"  the torch composition, forward + backward             {fmt(s['d_both_torch'])}   x {s['d_both_torch'][0] / s['d_both'][0]:.1f}")
    out.append("  (forward + backward includes the product with the incoming gradient, its sum and autograd's own work, the same on both sides)")
    del fns, kept_g, kept_d, q_leaf, d_leaf, g_n, g_d, depth
    torch.cuda.empty_cache()
    if "--only-passes" in sys.argv:
        return finish(out)

    # ---- 3. the training step of INTEGRATION.md 2a, with and without the normal-consistency term ----
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    with torch.no_grad():
        frame = render(GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0"), cam)[0]
    target = (frame + 0.1 * torch.randn((3, H, W), generator=gen).to(dev)).clamp_(0.0, 1.0)
    params, rast = GaussianParams.from_raw(*raw, device=dev), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)          # (a rate of 1e-6: the frame stays the frame)
    dens = DensityStats(params.num_gaussians, dev)

    def make_step(rs, slot, with_normals):
        def step():
            opt.zero_grad(set_to_none=True)
            if with_normals:
                color, dmap, omap, nmap = render(params, rs, cam, radii_slot=slot, depth=True, opacity_grad=True, normals=True)
                (photometric_loss(color, target) + 0.05 * normals.normal_consistency(nmap, dmap, omap, tan).mean()).backward()
            else:
                color, _, _ = render(params, rs, cam, radii_slot=slot)
                photometric_loss(color, target).backward()
            opt.step(slot.radii)
            dens.update(slot, W, H)
        return step
    steps = {}
    for name, wn in (("no normals (a)", False), ("normals=True (a)", True), ("no normals (b)", False), ("normals=True (b)", True)):
        steps[name] = lambda step=make_step(rast, FrameSlot(), wn): timed(step)
    res = interleaved(steps)
    out.append("one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii) + DensityStats.update()"
               " [+ 0.05 x the mean of normal_consistency: depth=True, opacity_grad=True, normals=True]")
    med = {}
    for name in steps:
        m = stats(res[name])
        med[name] = m[0]
        out.append(f"  {name:<34s}{fmt(m)}")
    plain = 0.5 * (med["no normals (a)"] + med["no normals (b)"])
    with_n = 0.5 * (med["normals=True (a)"] + med["normals=True (b)"])
    out.append(f"  with the normal term against without: {with_n - plain:+.3f} ms (the depth channel, the opacity map's gradient, the feature pass "
               f"at C = 3 and the torch operations of normal_consistency included); equal configurations differ by "
               f"{abs(med['no normals (a)'] - med['no normals (b)']):.3f} ms")

    # ---- 4. the default step against the parent commit's library ----
    out.append("the default step (no normals) through this tree's library and the parent commit's")
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
                   f"{lo:.3f} .. {hi:.3f} ms ({1e3 * (hi - lo):.1f} us): {'inside' if lo <= mine <= hi else 'OUTSIDE'}; equal configurations "
                   f"differ by {1e3 * abs(med['parent commit (a)'] - med['parent commit (b)']):.1f} us (parent) and "
                   f"{1e3 * abs(med['this tree (a)'] - med['this tree (b)']):.1f} us (this tree)")
    else:
        out.append("  parent commit: not measured (no --parent-lib)")
    finish(out)


if __name__ == "__main__":
    main()
