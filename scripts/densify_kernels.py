"""The densify kernels at the bench scene's size, for a kernel trace: 20 DensityStats.update over a frame with 52 % of the rows
visible and 6 densify_and_prune with a tenth of the Gaussians hot, on random values (no scene is built).
Usage: rocprofv3 --kernel-trace --stats -d DIR -o densify --output-format csv -- python scripts/densify_kernels.py
(profiles/densify_kernel_stats.txt: the library's rows of DIR/densify_kernel_stats.csv)"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gsrast_amd.autograd import FrameSlot  # noqa: E402
from gsrast_amd.densify import RAW, ROW_FLOATS, DensityStats, densify_and_prune  # noqa: E402
from gsrast_amd.optim import GaussianAdam  # noqa: E402

N = 5_834_784
dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(1)
rnd = lambda *shape: torch.randn(shape, generator=gen, device=dev)
base = {k: (rnd(N) if k == "opacity_logit" else rnd(N, ROW_FLOATS[k])) for k in RAW}
base["log_scale"] = base["log_scale"] - 4.0
moments = {k: (0.01 * torch.randn_like(base[k]), 0.01 * torch.rand_like(base[k])) for k in RAW}
slot = FrameSlot()
slot.radii = torch.where(torch.rand(N, generator=gen, device=dev) < 0.52, 7, 0).to(torch.int32)
slot.dL_dmean2D = 1e-5 * rnd(N, 2)
stats = DensityStats(N, dev)
for _ in range(20):
    stats.update(slot, 1920, 1080)
torch.cuda.synchronize()
keep = (torch.rand(N, generator=gen, device=dev), torch.ones(N, dtype=torch.int32, device=dev), stats.max_radii)


class Holder(torch.nn.Module):
    def __init__(self):
        super().__init__()
        for k in RAW:
            setattr(self, k, torch.nn.Parameter(base[k]))


for _ in range(6):
    p = Holder()
    opt = GaussianAdam(p.parameters(), lr=1e-6, eps=1e-15)
    for k in RAW:
        opt.state[getattr(p, k)].update(step=1, exp_avg=moments[k][0], exp_avg_sq=moments[k][1])
    st = DensityStats(0, dev)
    st.grad_accum, st.denom, st.max_radii = keep
    _, counts = densify_and_prune(p, opt, st, max_grad=0.9, extent=100.0 * float(torch.exp(torch.tensor(-3.15))))
torch.cuda.synchronize()
print("counts", counts)
