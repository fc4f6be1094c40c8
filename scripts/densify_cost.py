"""What adaptive density control costs on the bench scene (bench.py's own scene builder, 1920 x 1080, one GPU).

  the statistics   DensityStats.update (gsr_densify_accumulate) against the upstream trainer's three indexed torch ops over the
                   same frame (the gradients and radii of one render() + backward() with a FrameSlot)
  the step         render() + photometric_loss + backward() + GaussianAdam.step(radii) over one set of objects: with a
                   RadiiSlot twice (the two differ by the run-to-run spread only), with a FrameSlot, and with stats.update
  densification    gsr_densify_plan, gsr_densify_apply and the whole densify_and_prune (moments of all five arrays), against
                   the upstream procedure in torch ops — cat, boolean-mask indexing, bmm — handed the SAME masks ready made;
                   under the frame's own statistics, and under statistics that make a tenth of all Gaussians hot

percent_dense * extent = the median size, so that half of the hot Gaussians are cloned and half split. Bytes: what the
algorithm needs. Medians of device-event times, every configuration after its own warm-up, configurations interleaved round
by round. On a tree from before density control the script measures the step with a RadiiSlot alone.
Usage: python scripts/densify_cost.py [--reps N] [--splats N] [--out FILE]   (the table of profiles/densify_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
try:
    from gsrast_amd.autograd import FrameSlot  # noqa: E402
    from gsrast_amd.densify import RAW, DensityStats, densify_and_prune, plan_scalars  # noqa: E402
except ImportError:     # a tree from before density control: the step with a RadiiSlot alone (the baseline and its spread)
    FrameSlot = None
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
ROW_BYTES = 4 * (3 + 1 + 3 + 4 + 48)


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 20)
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
    return (f"  {what:<50s}{ms:8.3f} ms   {nbytes / 1e9:.3f} GB needed = {rate / 1e12:.2f} TB/s"
            f" = {100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak")


def medians(fns, reps, warm=3):
    for _ in range(warm):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def build_rotation(r):
    q = r / torch.sqrt((r * r).sum(dim=1))[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def torch_densify(t, m, clone, split, doomed_after, noise):
    """The upstream procedure over t = {name: tensor}, m = {name: (exp_avg, exp_avg_sq)} with its masks given: clone and split
    over the source rows, doomed_after over the rows after the split. -> the new tensors"""
    def extend(new):
        for k in RAW:
            t[k] = torch.cat((t[k], new[k]), dim=0)
            m[k] = tuple(torch.cat((a, torch.zeros_like(new[k])), dim=0) for a in m[k])

    def prune(mask):
        valid = ~mask
        for k in RAW:
            t[k] = t[k][valid]
            m[k] = tuple(a[valid] for a in m[k])

    extend({k: t[k][clone] for k in RAW})
    sel = torch.cat((split, torch.zeros(int(t["xyz"].shape[0]) - int(split.shape[0]), dtype=torch.bool, device=split.device)))
    stds = torch.exp(t["log_scale"][sel]).repeat(2, 1)
    samples = stds * noise
    rots = build_rotation(t["rotation"][sel]).repeat(2, 1, 1)
    new = {k: t[k][sel].repeat(2, *([1] * (t[k].dim() - 1))) for k in RAW}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][sel].repeat(2, 1)
    new["log_scale"] = torch.log(torch.exp(t["log_scale"][sel]).repeat(2, 1) / (0.8 * 2))
    extend(new)
    prune(torch.cat((sel, torch.zeros(2 * int(sel.sum()), dtype=torch.bool, device=sel.device))))
    prune(doomed_after)
    return t, m


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    make = lambda: GaussianParams.from_raw(*raw, device=dev)
    params = make()
    n = params.num_gaussians
    out = [f"densify cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds", f"bench frame ({label})"]

    # ---- the frame: target, gradients, radii, dL_dmean2D ----
    rast = SplatRasterizer(W, H, device="cuda:0")
    with torch.no_grad():
        frame = render(params, rast, cam)[0]
    target = (frame + 0.1 * torch.randn(frame.shape, generator=torch.Generator().manual_seed(7)).to(dev)).clamp_(0.0, 1.0)
    slot = FrameSlot() if FrameSlot else RadiiSlot()
    photometric_loss(render(params, rast, cam, radii_slot=slot)[0], target).backward()
    radii = slot.radii
    vis_mask = radii > 0
    vis = int(vis_mask.sum())
    out.append(f"N = {n}, visible {vis} ({100 * vis / n:.0f} %), R = {rast.last_num_rendered}, plan {rast.last_plan}")

    # ---- the statistics ----
    accumulate_ms = float("nan")
    if FrameSlot:
        grad2d = slot.dL_dmean2D
        stats = DensityStats(n, dev)
        t_acc, t_den, t_big = (torch.zeros_like(a) for a in (stats.grad_accum, stats.denom, stats.max_radii))
        ndc = torch.tensor([0.5 * W, 0.5 * H], device=dev)

        def torch_stats():
            t_big[vis_mask] = torch.max(t_big[vis_mask], radii[vis_mask])
            t_acc[vis_mask] += torch.norm(grad2d[vis_mask] * ndc, dim=-1)
            t_den[vis_mask] += 1

        m, _ = medians({"ours": lambda: stats.update(slot, W, H), "torch": torch_stats}, REPS)
        acc_bytes = 4 * n + 32 * vis
        out.append("the statistics of a frame (bytes: the radii word of every row; 20 read and 12 written per visible row)")
        out.append(rate_line("DensityStats.update (gsr_densify_accumulate)", m["ours"], acc_bytes))
        out.append(rate_line("torch, three indexed ops (the mask ready made)", m["torch"], acc_bytes))
        out.append(f"  torch takes {m['torch'] / m['ours']:.1f} x the time")
        accumulate_ms = m["ours"]
        del t_acc, t_den, t_big

    # ---- the step ----
    # One set of parameters, one rasterizer and one optimiser for every configuration (a rate of 1e-6: the frame stays the
    # frame): configurations built from objects of their own differ by 0.1 ms and more, in every round, through where their
    # memory happens to lie, which is more than what is to be measured here.
    p, r = make(), SplatRasterizer(W, H, device="cuda:0")
    opt = GaussianAdam(p.parameters(), lr=1e-6, eps=1e-15)
    st = DensityStats(n, dev) if FrameSlot else None

    def step(s, with_stats):
        def run():
            opt.zero_grad(set_to_none=True)
            photometric_loss(render(p, r, cam, radii_slot=s)[0], target).backward()
            opt.step(s.radii)
            if with_stats:
                st.update(s, W, H)
        return run

    steps = {"RadiiSlot, A": step(RadiiSlot(), False), "RadiiSlot, B": step(RadiiSlot(), False)}
    if FrameSlot:
        steps.update({"FrameSlot": step(FrameSlot(), False), "FrameSlot + stats.update": step(FrameSlot(), True)})
    m, span = medians(steps, 3 * REPS)
    base = min(m["RadiiSlot, A"], m["RadiiSlot, B"])
    out.append(f"one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii), medians of {3 * REPS} rounds")
    for k in steps:
        out.append(f"  {k:<50s}{m[k]:8.3f} ms ({m[k] - base:+.3f} ms; rounds {span[k][0]:.3f} .. {span[k][1]:.3f})")
    out.append(f"  the same configuration twice differs by {abs(m['RadiiSlot, A'] - m['RadiiSlot, B']):.3f} ms; the statistics alone take "
               f"{accumulate_ms:.3f} ms")
    del steps, p, r, opt, st
    torch.cuda.empty_cache()
    if FrameSlot:
        # the frame's own statistics: its gradient reaches few Gaussians of this scene (opaque splats in front hide the rest)
        stats = DensityStats(n, dev)
        stats.update(slot, W, H)
        g = stats.grad_accum / stats.denom.clamp(min=1)
        densification(out, "the frame's gradients, max_grad = the median of those that are not zero", params,
                      (stats.grad_accum, stats.denom, stats.max_radii), float(g[g > 0].median()), dev)
        # a tenth of all Gaussians hot, wherever they lie: gradients drawn uniformly, max_grad at their ninth decile
        drawn = torch.rand(n, generator=torch.Generator().manual_seed(11)).to(dev)
        densification(out, "uniform random gradients, max_grad = 0.9: a tenth of the Gaussians hot", params,
                      (drawn, torch.ones_like(stats.denom), stats.max_radii), 0.9, dev)
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


def densification(out, label, params, keep, max_grad, dev):
    """Plan, apply, the whole call and the torch composition under the statistics keep = (grad_accum, denom, max_radii)."""
    n = params.num_gaussians
    g = keep[0] / keep[1].clamp(min=1)
    sizes = params.log_scale.detach().max(dim=1).values
    extent = float(torch.exp(sizes.double()).median()) / 0.01
    kw = dict(max_grad=max_grad, min_opacity=0.005, extent=extent, max_screen_size=None, percent_dense=0.01)
    scalars = plan_scalars(max_grad, 0.005, extent, 0.01)
    base_raw = {k: getattr(params, k).detach() for k in RAW}
    base_m = {k: (0.01 * torch.randn_like(base_raw[k]), 0.01 * torch.rand_like(base_raw[k])) for k in RAW}
    # the masks, as the plan's definition gives them (no screen test)
    f32 = lambda v: float(np.float32(v))
    hot = g >= f32(scalars[0])
    big = sizes > f32(scalars[1])
    faint = base_raw["opacity_logit"] < f32(scalars[2])
    clone, split = hot & ~big, hot & big
    n_clone, n_split = int(clone.sum()), int(split.sum())
    doomed_after = torch.cat((faint[~split], faint[clone], faint[split], faint[split]))
    noise = torch.randn((2 * n_split, 3), device=dev)

    L = _capi.lib()
    stream = torch.cuda.current_stream(dev).cuda_stream
    temp = torch.empty(int(L.gsr_densify_plan_temp_bytes(n)), dtype=torch.uint8, device=dev)
    src_of, counts = torch.empty(3 * n, dtype=torch.int32, device=dev), torch.empty(4, dtype=torch.int32, device=dev)

    def plan():
        _capi.check(L.gsr_densify_plan(n, base_raw["opacity_logit"].data_ptr(), base_raw["log_scale"].data_ptr(), keep[0].data_ptr(),
                                       keep[1].data_ptr(), keep[2].data_ptr(), *scalars, 0, temp.data_ptr(), src_of.data_ptr(),
                                       counts.data_ptr(), stream), "gsr_densify_plan")

    plan()
    kept, clones, splits, total = (int(c) for c in counts.tolist())
    assert (clones, splits) == (int((clone & ~faint).sum()), int((split & ~faint).sum())), "the masks are not the plan's"
    out.append(f"densification, {label}: {n} -> {total} Gaussians ({kept} kept, {clones} clones, {splits} split into two)")
    dst = {k: torch.empty((total,) + tuple(base_raw[k].shape[1:]), device=dev) for k in RAW}
    dst_m = {k: (torch.empty_like(dst[k]), torch.empty_like(dst[k])) for k in RAW}
    child_noise = torch.randn((splits, 2, 3), device=dev)
    a = _capi.DensifyApplyArgs()
    a.struct_size, a.log_shrink, a.n_src = C.sizeof(_capi.DensifyApplyArgs), scalars[4], n
    a.counts[:] = [kept, clones, splits, total]
    a.src_of, a.noise, a.stream = src_of.data_ptr(), child_noise.data_ptr(), stream
    for k in RAW:
        arr = getattr(a, k)
        arr.src, arr.src_exp_avg, arr.src_exp_avg_sq = base_raw[k].data_ptr(), base_m[k][0].data_ptr(), base_m[k][1].data_ptr()
        arr.dst, arr.dst_exp_avg, arr.dst_exp_avg_sq = dst[k].data_ptr(), dst_m[k][0].data_ptr(), dst_m[k][1].data_ptr()
    apply = lambda: _capi.check(L.gsr_densify_apply(C.byref(a)), "gsr_densify_apply")

    class Holder(torch.nn.Module):                           # densify_and_prune replaces the five attributes: a fresh holder per call
        def __init__(self):
            super().__init__()
            for k in RAW:
                setattr(self, k, torch.nn.Parameter(base_raw[k]))

    def whole():
        p = Holder()
        opt = GaussianAdam(p.parameters(), lr=1e-6, eps=1e-15)
        for k in RAW:
            opt.state[getattr(p, k)].update(step=1, exp_avg=base_m[k][0], exp_avg_sq=base_m[k][1])
        st = DensityStats(0, dev)
        st.grad_accum, st.denom, st.max_radii = keep
        densify_and_prune(p, opt, st, **kw)

    def upstream():
        torch_densify(dict(base_raw), dict(base_m), clone, split, doomed_after, noise)

    m, _ = medians({"plan": plan, "apply": apply, "whole": whole, "torch": upstream}, max(5, REPS // 2), warm=2)
    plan_bytes = n * (4 + 12 + 12) + 3 * n * 4 * 5 + 4 * total
    apply_bytes = ROW_BYTES * (2 * total + 2 * kept + 2 * total) + 5 * 4 * total
    out.append("  (bytes: plan = its inputs, the flags written, read twice by the scan, written and read again, src_of; apply = every"
               " parameter row read and written, the kept rows' moments read, every moment row written, src_of per array)")
    out.append(rate_line("gsr_densify_plan (classify, scan, scatter)", m["plan"], plan_bytes))
    out.append(rate_line("gsr_densify_apply, with moments", m["apply"], apply_bytes))
    out.append(f"  {'densify_and_prune, whole (allocations, one sync)':<50s}{m['whole']:8.3f} ms")
    out.append(f"  {'the upstream procedure in torch ops, masks given':<50s}{m['torch']:8.3f} ms = {m['torch'] / m['whole']:.1f} x densify_and_prune")


if __name__ == "__main__":
    main()
