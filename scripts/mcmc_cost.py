"""What the three steps of 3DGS-MCMC cost on the bench scene (bench.py's own scene builder, 1920 x 1080, one GPU).

  the noise        inject_noise (gsr_mcmc_noise) against the same update composed of torch ops (sigmoid, exp, the nine rotation
                   entries, two 3 x 3 products per row: with bmm, as upstream writes it, and with broadcast products), all handed the
                   same noise tensor; and inject_noise drawing its own
  the step         render() + photometric_loss + backward() + GaussianAdam.step(radii) of profiles/photo_loss_cost.txt over
                   one set of objects: twice without (the two differ by the run-to-run spread only) and once with inject_noise
  relocation       relocate_dead and add_new with 1 % of the Gaussians made dead, against the procedure in torch ops — bincount,
                   the relocation formula in float64 from a table of its coefficients, indexed assignments, cat — handed the
                   SAME samples ready made (it draws nothing and plans nothing)

Bytes: what the algorithm needs. Medians of device-event times, every configuration after its own warm-up, configurations
interleaved round by round; what a configuration needs put back before a round (the dead rows) is outside its events.
Usage: python scripts/mcmc_cost.py [--reps N] [--splats N] [--out FILE]   (the table of profiles/mcmc_cost.txt)"""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from gsrast_amd import camera, mcmc  # noqa: E402
from gsrast_amd.autograd import GaussianParams, RadiiSlot, render  # noqa: E402
from gsrast_amd.densify import RAW  # noqa: E402
from gsrast_amd.loss import photometric_loss  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
NOISE_ROW_BYTES = 68       # xyz read and written, opacity_logit, log_scale, rotation and noise read
MIN_OPACITY = 0.005
MAX_RATIO = 51


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


def medians(fns, reps, warm=3, before=None):
    """fns: {name: callable}; before: {name: callable run ahead of every call of that name, outside its events}."""
    before = before or {}
    def once(k, fn, clock):
        if k in before:
            before[k]()
        return timed(fn) if clock else fn()
    for _ in range(warm):
        for k, fn in fns.items():
            once(k, fn, False)
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(once(k, fn, True))
    return {k: float(np.median(v)) for k, v in ms.items()}, {k: (float(np.min(v)), float(np.max(v))) for k, v in ms.items()}


def build_rotation(r):
    q = r / torch.sqrt((r * r).sum(dim=1))[:, None]
    R = torch.zeros((q.size(0), 3, 3), device=r.device)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


@torch.no_grad()
def torch_noise(p, noise, scaler):
    """The upstream trainer's inject_noise_to_position in torch ops."""
    o = torch.sigmoid(p.opacity_logit)
    gate = torch.sigmoid(100.0 * ((1.0 - o) - 0.995)) * scaler
    L = build_rotation(p.rotation) * torch.exp(p.log_scale)[:, None, :]
    cov = torch.bmm(L, L.transpose(1, 2))
    p.xyz.add_(torch.bmm(cov, (noise * gate[:, None]).unsqueeze(-1)).squeeze(-1))


@torch.no_grad()
def torch_noise_elementwise(p, noise, scaler):
    """The same update without bmm: broadcast products and sums over N x 3 x 3 temporaries."""
    o = torch.sigmoid(p.opacity_logit)
    v = noise * (torch.sigmoid(100.0 * ((1.0 - o) - 0.995)) * scaler)[:, None]
    R, s = build_rotation(p.rotation), torch.exp(p.log_scale)
    w = (R * v[:, :, None]).sum(dim=1) * s * s
    p.xyz.add_((R * w[:, None, :]).sum(dim=2))


def relocation_table(dev):
    """T[r - 1][k] = sum over i = 1..r of C(i - 1, k) (-1)^k / sqrt(k + 1): D(ratio r) = sum_k T[r - 1][k] o_new^(k + 1)."""
    t = np.zeros((MAX_RATIO, MAX_RATIO))
    for i in range(1, MAX_RATIO + 1):
        for k in range(i):
            t[i - 1, k] = math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1.0)
    return torch.from_numpy(np.cumsum(t, axis=0)).to(dev)


@torch.no_grad()
def torch_update(t, m, sampled, table):
    """Steps 1 and 2 of gsr_mcmc_relocate in torch ops, float64 (a row drawn twice is written twice with the same values)."""
    n = t["xyz"].shape[0]
    ratio = (torch.bincount(sampled, minlength=n)[sampled] + 1).clamp_(max=MAX_RATIO)
    o = torch.sigmoid(t["opacity_logit"][sampled]).double()
    o_new = -torch.expm1(torch.log1p(-o) / ratio)
    powers = o_new[:, None] ** torch.arange(1, MAX_RATIO + 1, device=o.device, dtype=torch.float64)
    D = (powers * table[ratio - 1]).sum(dim=1)
    o_c = o_new.clamp(MIN_OPACITY, 1.0 - 2.0 ** -23)
    t["opacity_logit"][sampled] = torch.log(o_c / (1.0 - o_c)).float()
    t["log_scale"][sampled] = t["log_scale"][sampled] + torch.log(o / D).float()[:, None]
    for k in RAW:
        for a in m[k]:
            a[sampled] = 0


@torch.no_grad()
def torch_relocate(t, m, sampled, dead_idx, table):
    torch_update(t, m, sampled, table)
    for k in RAW:
        t[k][dead_idx] = t[k][sampled]
        for a in m[k]:
            a[dead_idx] = 0


@torch.no_grad()
def torch_add_new(t, m, sampled, table):
    torch_update(t, m, sampled, table)
    new = {k: torch.cat((t[k], t[k][sampled]), dim=0) for k in RAW}
    new_m = {k: tuple(torch.cat((a, torch.zeros_like(t[k][sampled])), dim=0) for a in m[k]) for k in RAW}
    return new, new_m


class Holder(torch.nn.Module):
    """The five arrays as parameters over given tensors (add_new replaces the attributes: a fresh holder per call)."""

    def __init__(self, tensors):
        super().__init__()
        for k in RAW:
            setattr(self, k, torch.nn.Parameter(tensors[k]))


def main():
    dev = torch.device("cuda:0")
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    o = np.clip(sc["opacities"].astype(np.float64), 1e-6, 1.0 - 1e-6)
    raw = (sc["means3D"][:, :3], np.log(o / (1.0 - o)), np.log(sc["scales"][:, :3].astype(np.float64)), sc["rotations"], sc["shs"])
    make = lambda: GaussianParams.from_raw(*raw, device=dev)
    params = make()
    n = params.num_gaussians
    out = [f"mcmc cost, {W} x {H}, {torch.cuda.get_device_name(0)}, medians of {REPS} rounds", f"bench frame ({label})", f"N = {n}"]

    # ---- the noise (a scaler of 0: the positions, and so every round, stay the same; the kernel's work does not depend on it) ----
    noise = torch.randn((n, 3), device=dev)
    m, span = medians({"ours": lambda: mcmc.inject_noise(params, 0.0, noise=noise), "torch": lambda: torch_noise(params, noise, 0.0),
                       "torch, elementwise": lambda: torch_noise_elementwise(params, noise, 0.0),
                       "ours, drawing": lambda: mcmc.inject_noise(params, 0.0)}, REPS)
    nbytes = NOISE_ROW_BYTES * n
    rate = nbytes / (m["ours"] * 1e-3)
    out.append(f"the noise of one step ({NOISE_ROW_BYTES} bytes per row: {nbytes / 1e6:.0f} MB)")
    out.append(f"  {'inject_noise (gsr_mcmc_noise), noise given':<50s}{m['ours']:8.3f} ms = {rate / 1e12:.2f} TB/s = "
               f"{100 * rate / HBM_PEAK:.0f} % of the 8 TB/s peak (rounds {span['ours'][0]:.3f} .. {span['ours'][1]:.3f})")
    out.append(f"  {'the same update in torch ops (bmm, as upstream)':<50s}{m['torch']:8.3f} ms = {m['torch'] / m['ours']:.0f} x")
    out.append(f"  {'... with broadcast products in place of bmm':<50s}{m['torch, elementwise']:8.3f} ms = {m['torch, elementwise'] / m['ours']:.0f} x")
    out.append(f"  {'inject_noise drawing torch.randn((N, 3)) itself':<50s}{m['ours, drawing']:8.3f} ms")
    noise_ms = m["ours"]

    # ---- the step ----
    rast = SplatRasterizer(W, H, device="cuda:0")
    with torch.no_grad():
        frame = render(params, rast, cam)[0]
    target = (frame + 0.1 * torch.randn(frame.shape, generator=torch.Generator().manual_seed(7)).to(dev)).clamp_(0.0, 1.0)
    opt = GaussianAdam(params.parameters(), lr=1e-6, eps=1e-15)
    slot = RadiiSlot()

    def step(with_noise):
        def run():
            opt.zero_grad(set_to_none=True)
            photometric_loss(render(params, rast, cam, radii_slot=slot)[0], target).backward()
            opt.step(slot.radii)
            if with_noise:
                mcmc.inject_noise(params, 0.0, noise=noise)
        return run

    m, span = medians({"without, A": step(False), "without, B": step(False), "with inject_noise": step(True)}, 3 * REPS)
    base = min(m["without, A"], m["without, B"])
    out.append(f"one training step: render() + photometric_loss + backward() + GaussianAdam.step(radii), medians of {3 * REPS} rounds")
    for k in m:
        out.append(f"  {k:<50s}{m[k]:8.3f} ms ({m[k] - base:+.3f} ms; rounds {span[k][0]:.3f} .. {span[k][1]:.3f})")
    out.append(f"  the same configuration twice differs by {abs(m['without, A'] - m['without, B']):.3f} ms; the noise alone takes {noise_ms:.3f} ms")
    del opt, rast, slot
    torch.cuda.empty_cache()

    # ---- relocation: 1 % dead ----
    gen = torch.Generator().manual_seed(3)
    dead_rows = torch.randperm(n, generator=gen)[: n // 100].sort().values.to(dev)
    base_t = {k: getattr(params, k).detach() for k in RAW}
    base_m = {k: (0.01 * torch.randn_like(base_t[k]), 0.01 * torch.rand_like(base_t[k])) for k in RAW}
    live_logit = base_t["opacity_logit"].clone()

    def kill():
        base_t["opacity_logit"].copy_(live_logit)
        base_t["opacity_logit"][dead_rows] = -10.0

    kill()
    weights = torch.sigmoid(base_t["opacity_logit"]) * (base_t["opacity_logit"] > math.log(MIN_OPACITY / (1.0 - MIN_OPACITY)))
    dead_idx = torch.nonzero(weights == 0).squeeze(1)
    sampled = mcmc.sample_rows(weights, torch.rand(dead_idx.numel(), dtype=torch.float64, generator=gen).to(dev))
    grow = int(1.05 * n) - n
    grown = mcmc.sample_rows(torch.sigmoid(live_logit), torch.rand(grow, dtype=torch.float64, generator=gen).to(dev))
    table = relocation_table(dev)
    moved = []

    def holder_and_opt():
        p = Holder(base_t)
        opt = GaussianAdam(p.parameters(), lr=1e-6, eps=1e-15)
        for k in RAW:
            opt.state[getattr(p, k)].update(step=1, exp_avg=base_m[k][0], exp_avg_sq=base_m[k][1])
        return p, opt

    def ours_relocate():
        p, opt = holder_and_opt()
        moved.append(mcmc.relocate_dead(p, opt, min_opacity=MIN_OPACITY))

    def ours_add():
        p, opt = holder_and_opt()
        moved.append(mcmc.add_new(p, opt, cap_max=2 * n, min_opacity=MIN_OPACITY))

    fns = {"relocate_dead": ours_relocate, "torch relocate": lambda: torch_relocate(base_t, base_m, sampled, dead_idx, table),
           "add_new": ours_add, "torch add_new": lambda: torch_add_new(base_t, base_m, grown, table)}
    m, _ = medians(fns, max(5, REPS // 2), warm=2, before={k: kill for k in fns})
    assert set(moved) <= {int(dead_idx.numel()), grow} and len(set(moved)) == 2, (set(moved), int(dead_idx.numel()), grow)
    out.append(f"relocation, 1 % of the rows made dead beside the scene's own faint ones ({100 * dead_idx.numel() / n:.1f} % dead): "
               f"{dead_idx.numel()} rows moved onto {int(torch.unique(sampled).numel())} distinct live rows; "
               f"growth by 5 %: {grow} rows from {int(torch.unique(grown).numel())} distinct rows; moments of all five arrays")
    out.append(f"  {'relocate_dead, whole (plan, one sync, draw, sample)':<50s}{m['relocate_dead']:8.3f} ms")
    out.append(f"  {'the procedure in torch ops, samples given':<50s}{m['torch relocate']:8.3f} ms = {m['torch relocate'] / m['relocate_dead']:.1f} x")
    out.append(f"  {'add_new, whole (weights, draw, sample, gather)':<50s}{m['add_new']:8.3f} ms")
    out.append(f"  {'the procedure in torch ops, samples given':<50s}{m['torch add_new']:8.3f} ms = {m['torch add_new'] / m['add_new']:.1f} x")
    print("\n".join(out), flush=True)
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
