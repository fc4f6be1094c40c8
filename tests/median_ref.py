"""Reference of the median map and the per-pixel Gaussian ids (include/gsrast_amd_median.h), shared by tests/test_median_cpu.py
and tests/test_gpu_median.py with the scenes of tests/contrib_ref.py (all_scenes, LIST_LENGTHS: imported), so that what the CPU
file establishes of a scene holds for the arrays the GPU file compares.

forward: a float32 numpy restatement of the header's forward, line for line, as hooks of walk_ref.replay (the
masks, the operation order, exp = the C++ oracle's libm expf, the cut-off: written once there): sel, dom and the gathered value per pixel, and
beside them where in its tile's list the selected record stands and the pixel's first and last blended records — what the
blindness guards ask. The GPU's three maps are compared with it bit for bit.
backward: the header's sum in float64 (np.add.at), with the sum of |g| per Gaussian for the bound.
depth_gradients64: the "depth" composition of autograd.rasterize in float64 torch, fed a map of ids."""
import types

import numpy as np

import walk_ref
from contrib_ref import LIST_LENGTHS, all_scenes      # noqa: F401  (the scenes both files use)
from walk_ref import T_CUTOFF, depth_values, ulp32    # noqa: F401  (depth_values: the view-space z as autograd._distortion_values forms it)

F = np.float32
NONE = np.uint32(0xFFFFFFFF)
FIRST_HIT = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
THRESHOLDS = (0.5, 0.05, 0.0, FIRST_HIT)


def forward(means2D, conic_opacity, ranges, lists, values, W, H, threshold, t_cutoff=0.001, tile_rows=None, exp=None):
    """out [H,W] float32, ids / dominant_ids [H,W] uint32, finalT, nContrib [H,W] of the replay over the tiles of rows `tile_rows`
    (default: all; 0 / NONE / zeros outside), and per pixel the 1-based list positions sel_pos, first_pos, last_pos of the
    selected, the first and the last blended record (0: none) and blended, how many it blended. values: [N] or None (out zeros)."""
    thr = F(threshold)
    assert F(0.0) <= thr < F(1.0), threshold
    ids, dom_ids = np.full((H, W), NONE, np.uint32), np.full((H, W), NONE, np.uint32)
    pos = {k: np.zeros((H, W), np.int64) for k in ("sel_pos", "first_pos", "last_pos", "blended")}
    scale = F(4294967296.0)

    def start(tx, ty):
        return types.SimpleNamespace(sel=np.full(256, NONE, np.uint32), dom=np.full(256, NONE, np.uint32), best=np.zeros(256, np.uint32),
                                     sel_pos=np.zeros(256, np.int64), first_pos=np.zeros(256, np.int64), count=np.zeros(256, np.int64))

    def record(r, g, at, con, dx, dy, power, alpha, T, upd):
        take = upd & (T > thr)                           # T: the transmittance in front of the record
        r.sel[take] = g
        r.sel_pos[take] = at
        w = (alpha * T).astype(F)
        q = np.trunc((w * scale).astype(F).astype(np.float64)).astype(np.uint64).astype(np.uint32)
        better = upd & (q > r.best)                      # strict: a tie stays in front, q == 0 never wins
        r.best[better] = q[better]
        r.dom[better] = g
        r.first_pos[upd & (r.count == 0)] = at
        r.count[upd] += 1

    def end(r, px, py, inside, T, last, done):
        ys, xs = py[inside], px[inside]
        ids[ys, xs] = r.sel[inside]
        dom_ids[ys, xs] = r.dom[inside]
        for key, v in (("sel_pos", r.sel_pos), ("first_pos", r.first_pos), ("last_pos", last), ("blended", r.count)):
            pos[key][ys, xs] = v[inside]

    finalT, ncontrib, _ = walk_ref.replay(means2D, conic_opacity, ranges, lists, W, H, t_cutoff, tile_rows, exp, start, record, end)
    out = np.zeros((H, W), F)
    if values is not None:
        val = np.asarray(values, F).reshape(-1)
        hit = ids != NONE
        out[hit] = val[ids[hit]]                                         # a gather: the value's bits
    return dict(out=out, ids=ids, dominant_ids=dom_ids, finalT=finalT, nContrib=ncontrib, **pos)


def of_state(state, cam, values, threshold, semantics="gscuda", tile_rows=None):
    """forward() over a forward state (cpu_oracle.forward's dict, or the arrays read back from the GPU under those names)."""
    return forward(state["means2D"], state["conicOpacity"], state["ranges"], state["values"], values, cam.width, cam.height, threshold,
                   T_CUTOFF[semantics], tile_rows)


def backward(ids, g, n, tile_rows=None):
    """(dL_dvalues float64 [n], sum of |g| per row float64 [n], pixels per row) of L = sum g out with the selection fixed: an id
    >= n, NONE included, is dropped; tile_rows: only those rows of tiles count."""
    ids = np.asarray(ids).view(np.uint32).astype(np.int64)
    g = np.asarray(g, np.float64)
    if tile_rows is not None:
        rows = np.zeros(ids.shape, bool)
        rows[16 * tile_rows[0]:16 * tile_rows[1]] = True
    else:
        rows = np.ones(ids.shape, bool)
    keep = rows & (ids < n)
    sums, mags, pixels = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.int64)
    np.add.at(sums, ids[keep], g[keep])
    np.add.at(mags, ids[keep], np.abs(g[keep]))
    np.add.at(pixels, ids[keep], 1)
    return sums, mags, pixels


def backward_bound(sums, mags):
    """|got - ref| <= ulp32(ref) + 2^-32 sum |g|: at most 2^21 double additions of the row's terms (each off by at most 2^-53 of
    the running magnitude, which sum |g| bounds), then one rounding to float32 (half an ulp; one whole ulp is allowed)."""
    return ulp32(sums) + 2.0 ** -32 * mags


def exact_gradient(cam, seed=41):
    """[H,W] float32 in multiples of 2^-10 with |g| <= 1: every double sum of them is exact, whatever the order."""
    rng = np.random.default_rng(seed + 1000 * cam.width + cam.height)
    return (rng.integers(-1024, 1025, (cam.height, cam.width)).astype(np.float64) / 1024.0).astype(F)


def random_gradient(cam, seed=43):
    return np.random.default_rng(seed + 1000 * cam.width + cam.height).normal(size=(cam.height, cam.width)).astype(F)


def random_values(n, seed=47):
    return np.random.default_rng(seed + n).normal(size=n).astype(F)


def depth_gradients64(means3D, view, ids, g):
    """The "depth" composition in float64 torch, fed a map of ids: L = sum_p g(p) z[ids[p]] over the pixels that selected a
    record. Returns (dL_dmeans3D [N,4], dL_dview [16]) as float64 numpy."""
    import torch
    m = torch.tensor(np.asarray(means3D, np.float64), dtype=torch.float64, requires_grad=True)
    v = torch.tensor(np.asarray(view, np.float64).reshape(-1), dtype=torch.float64, requires_grad=True)
    z = (m[:, 0] * v[2] + m[:, 1] * v[6]) + (m[:, 2] * v[10] + v[14])
    ids = np.asarray(ids).view(np.uint32).astype(np.int64)
    hit = ids < m.shape[0]
    idx = torch.from_numpy(ids[hit])
    loss = (torch.from_numpy(np.asarray(g, np.float64)[hit]) * z[idx]).sum()
    loss.backward()
    return m.grad.numpy(), v.grad.numpy()
