"""The reference of adaptive density control (gsr_densify_accumulate / _plan / _apply), in numpy, written the way the upstream
trainer does it: boolean masks and np.concatenate — clone, then split, then prune — not a scan and a gather. The arithmetic
is in the dtype of the arrays passed: float32 states what the kernels must give bit for bit, float64 is compared with a
literal transcription of the upstream procedure (tests/test_densify_cpu.py).

The standard deviations and the normalised quaternions of the Gaussians are INPUTS (`stds` [N,3], `quats` [N,4], real part
first): the GPU tests feed them from gsrast_amd.autograd.activate, whose bits are those of the kernel's own exp and
normalisation by construction, so that no exponential is compared across implementations.
"""
import math

import numpy as np

RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
WIDTHS = {"xyz": 3, "opacity_logit": 1, "log_scale": 3, "rotation": 4, "shs": 48}


def plan_scalars(max_grad, min_opacity, extent, percent_dense=0.01, dtype=np.float32):
    """(max_grad, log_dense, logit_min_opacity, log_world, log_shrink): doubles, each rounded to `dtype` once."""
    vals = (max_grad, math.log(percent_dense * extent), math.log(min_opacity / (1.0 - min_opacity)), math.log(0.1 * extent),
            math.log(0.8 * 2))
    return tuple(dtype(v) for v in vals)


def accumulate(grad, radii, half_width, half_height, grad_accum, denom, max_radii):
    """One frame added to the three statistics -> new arrays. A row with radii <= 0 keeps its bits; its gradient is not used."""
    on = radii > 0
    g = np.where(on[:, None], grad, 0).astype(np.float32)
    gx, gy = g[:, 0] * np.float32(half_width), g[:, 1] * np.float32(half_height)
    norm = np.sqrt(gx * gx + gy * gy).astype(np.float32)
    acc = grad_accum.copy()
    acc[on] = (grad_accum + norm)[on]
    return acc, np.where(on, denom + 1, denom).astype(np.int32), np.where(on, np.maximum(max_radii, radii), max_radii).astype(np.int32)


def build_rotation(q):
    """Upstream's build_rotation of already normalised quaternions (r, x, y, z) -> [n,3,3], in q's dtype."""
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    one, two = q.dtype.type(1), q.dtype.type(2)
    R = np.empty((q.shape[0], 3, 3), q.dtype)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - r * z)
    R[:, 0, 2] = two * (x * z + r * y)
    R[:, 1, 0] = two * (x * y + r * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - r * x)
    R[:, 2, 0] = two * (x * z - r * y)
    R[:, 2, 1] = two * (y * z + r * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def mean_gradient(grad_accum, denom):
    """grad_accum / denom, 0 where never seen, and 0 for a NaN (upstream: grads[grads.isnan()] = 0.0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(denom > 0, grad_accum / denom.astype(grad_accum.dtype), grad_accum.dtype.type(0))
    g[np.isnan(g)] = 0
    return g


def densify(raw, moments, grad_accum, denom, max_radii, scalars, max_screen, noise, stds, quats):
    """raw: {name: array} of the five raw arrays; moments: {name: (exp_avg, exp_avg_sq)} for the arrays that have them.
    scalars: plan_scalars(...) in the arrays' dtype; max_screen: int, <= 0 = off. noise [S,2,3]: that of the split parents whose
    children survive, in source order (S is not known before the call: pass more rows, the first S are used).
    -> dict: raw, moments (the new arrays), src_of i32[N_new], counts (K, C, S, N_new), and the masks over the SOURCE rows
    kept, clone, split (every split parent), doomed, child_doomed (of the split parents: their children go)."""
    max_grad, log_dense, logit_min, log_world, log_shrink = scalars
    assert max_grad > 0                                   # (upstream pads the clones' gradients with zeros: they must not be hot)
    dt = raw["xyz"].dtype
    n = raw["xyz"].shape[0]
    P = {k: raw[k].reshape(n, WIDTHS[k]) for k in RAW}
    M = {k: tuple(a.reshape(n, WIDTHS[k]) for a in moments[k]) for k in moments}
    g = mean_gradient(grad_accum, denom)
    src = np.arange(n, dtype=np.int32)
    radii = max_radii.copy()

    def append(new, new_src):
        nonlocal src, radii
        for k in RAW:
            P[k] = np.concatenate([P[k], new[k]])
            if k in M:
                M[k] = tuple(np.concatenate([a, np.zeros_like(new[k])]) for a in M[k])
        src = np.concatenate([src, new_src.astype(np.int32)])
        radii = np.concatenate([radii, max_radii[new_src]])               # a new row is tested with its parent's radius

    def prune(mask):
        nonlocal src, radii
        keep = ~mask
        for k in RAW:
            P[k] = P[k][keep]
            if k in M:
                M[k] = tuple(a[keep] for a in M[k])
        src, radii = src[keep], radii[keep]

    # ---- densify_and_clone ----
    big = P["log_scale"].max(axis=1) > log_dense
    clone = (g >= max_grad) & ~big
    append({k: P[k][clone] for k in RAW}, np.nonzero(clone)[0])
    # ---- densify_and_split ----
    padded = np.zeros(P["xyz"].shape[0], dt)
    padded[:n] = g
    split_all = (padded >= max_grad) & (P["log_scale"].max(axis=1) > log_dense)
    split = split_all[:n]
    assert not split_all[n:].any()
    parents = np.nonzero(split)[0]
    # the noise is drawn for the parents whose children survive the pruning below: the same test, on the children's values
    faint = P["opacity_logit"][:n, 0] < logit_min
    sized = (lambda m: (max_radii > max_screen) | (m > log_world)) if max_screen > 0 else (lambda m: np.zeros(n, bool))
    m_src = raw["log_scale"].reshape(n, 3).max(axis=1)
    doomed = faint | sized(m_src)
    child_doomed = faint | sized((raw["log_scale"].reshape(n, 3) - log_shrink).max(axis=1))
    survive = ~child_doomed[parents]
    s_count = int(survive.sum())
    z = np.zeros((parents.size, 2, 3), dt)
    z[survive] = noise[:s_count]
    st, R = stds[parents].astype(dt), build_rotation(quats[parents].astype(dt))
    children = []
    for k in (0, 1):
        d = st * z[:, k, :]
        moved = np.stack([(R[:, a, 0] * d[:, 0] + R[:, a, 1] * d[:, 1]) + R[:, a, 2] * d[:, 2] for a in range(3)], axis=1)
        child = {name: P[name][parents] for name in RAW}
        child["xyz"] = P["xyz"][parents] + moved
        child["log_scale"] = P["log_scale"][parents] - log_shrink
        children.append(child)
    n_before = P["xyz"].shape[0]
    append({name: np.concatenate([children[0][name], children[1][name]]) for name in RAW}, np.concatenate([parents, parents]))
    prune(np.concatenate([split_all, np.zeros(2 * parents.size, bool)]))
    assert P["xyz"].shape[0] == n_before + parents.size
    # ---- prune ----
    mask = P["opacity_logit"][:, 0] < logit_min
    if max_screen > 0:
        mask = mask | (radii > max_screen) | (P["log_scale"].max(axis=1) > log_world)
    prune(mask)
    total = P["xyz"].shape[0]
    kept = ~split & ~doomed
    counts = (int(kept.sum()), int((clone & ~doomed).sum()), s_count, total)
    assert counts[0] + counts[1] + 2 * counts[2] == total
    out_raw = {k: (P[k].reshape(total) if k == "opacity_logit" else P[k]) for k in RAW}
    out_mom = {k: tuple(a.reshape(total) if k == "opacity_logit" else a for a in M[k]) for k in M}
    return dict(raw=out_raw, moments=out_mom, src_of=src, counts=counts, kept=kept, clone=clone & ~doomed, split=split,
                doomed=doomed, child_doomed=split & child_doomed)


def seeded_case(n, seed, with_screen=True):
    """The scene the GPU tests use at `n` rows: raw arrays, moments, statistics and thresholds under which every class
    occurs (tests/test_densify_cpu.py asserts that on this reference alone). -> dict"""
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.normal(size=shape).astype(np.float32)
    extent = 4.0
    scalars = plan_scalars(2e-4, 0.005, extent)
    raw = {"xyz": f(n, 3), "opacity_logit": (2.0 * f(n) - 3.0).astype(np.float32), "rotation": f(n, 4), "shs": f(n, 48)}
    # log-scales around log_dense (clone / split), a few beyond log_world and between log_world and log_world + log_shrink
    ls = (float(scalars[1]) - 0.5 + 0.8 * f(n, 3)).astype(np.float32)
    far = rng.random(n) < 0.15
    ls[far, 0] = (float(scalars[3]) + rng.uniform(-0.3, 0.9, int(far.sum()))).astype(np.float32)
    raw["log_scale"] = ls
    moments = {k: ((0.1 * f(*raw[k].shape)).astype(np.float32), (10.0 ** rng.uniform(-4, 0, raw[k].shape)).astype(np.float32)) for k in RAW}
    denom = rng.integers(0, 5, n).astype(np.int32)
    grad_accum = (denom * 2e-4 * 10.0 ** rng.uniform(-1, 1, n)).astype(np.float32)
    grad_accum[rng.random(n) < 0.05] = np.nan
    max_radii = rng.integers(0, 40, n).astype(np.int32)
    if n <= 2:                                            # (the smallest scenes cannot hold every class: row 0 splits, row 1 clones)
        raw["opacity_logit"][:] = 1.0
        raw["log_scale"][:] = float(scalars[1]) - 1.0
        raw["log_scale"][0, 1] = float(scalars[1]) + 0.5
        denom[:], grad_accum[:], max_radii[:] = 2, 1.0, 5
    noise = f(n, 2, 3)
    return dict(raw=raw, moments=moments, grad_accum=grad_accum, denom=denom, max_radii=max_radii, scalars=scalars,
                max_screen=30 if with_screen else 0, noise=noise, extent=extent)
