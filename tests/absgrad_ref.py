"""Reference of the absolute screen-space gradient (include/gsrast_amd_absgrad.h): float64, tile-vectorised [L records x 256
pixels] the way oracle/backward_np.blend_tile_backward is, over the forward's float32 decisions (its f32_forward=True semantics:
power, exp = libm's expf, alpha and the transmittance product in float32 in the forward's operation order; the sums in float64).
It takes C channels — (r, g, b) or (r, g, b, d) — with a pixel gradient per channel, a background per channel and an optional
seed for the accumulated opacity, so that the three terms of L enter one dL/dalpha per pixel as they do in the kernel.
Shared by tests/test_absgrad_cpu.py and tests/test_gpu_absgrad.py, with the scenes and the pixel gradients both files use."""
import functools

import numpy as np

TILE = 16
T_CUTOFF = {"gscuda": 0.001, "inria": 0.0001}


def tile_absgrad(xy, co, chan, tx, ty, width, height, background, g_tile, g_alpha_tile=None, t_cutoff=0.001):
    """One 16 x 16 tile. xy [L,2], co [L,4], chan [L,C]: the records of the tile's list, front to back; background [C];
    g_tile [C,16,16] and g_alpha_tile [16,16] or None (entries outside the image are ignored).
    Returns per record: signed [L,2] (the render backward's d_mean), A [L,2] (the sum over pixels of |share|), M [L,2] (the
    condition scale: the same sum with every factor replaced by its absolute value — dL/dalpha becomes |T_before cg| +
    |behind / (1 - alpha)|, cg and `behind` themselves sums of absolute values, the opacity seed entering as |g_a|), k [L] (the
    walk depth), pixels / free_pixels [L]; per pixel final_t, n_contrib [16,16]."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    co = np.asarray(co, np.float64).reshape(-1, 4)
    chan = np.asarray(chan, np.float64)
    chan = chan.reshape(xy.shape[0], -1)
    bg = np.asarray(background, np.float64)
    L, C = chan.shape
    assert bg.shape == (C,), (bg.shape, C)
    ys, xs = np.mgrid[0:TILE, 0:TILE]
    px = (tx * TILE + xs).reshape(-1).astype(np.float64)
    py = (ty * TILE + ys).reshape(-1).astype(np.float64)
    inside = (px < width) & (py < height)
    gp = np.asarray(g_tile, np.float64).reshape(C, -1) * inside[None, :]
    ga = np.zeros(px.size) if g_alpha_tile is None else np.asarray(g_alpha_tile, np.float64).reshape(-1) * inside
    if L == 0:
        z2, zi = np.zeros((0, 2)), np.zeros(0, np.int64)
        return {"signed": z2, "A": z2.copy(), "M": z2.copy(), "k": zi, "pixels": zi.copy(), "free_pixels": zi.copy(),
                "final_t": inside.astype(np.float64).reshape(TILE, TILE), "n_contrib": np.zeros((TILE, TILE), np.int64)}
    from oracle import cpu_oracle
    f = np.float32
    dx = xy[:, 0:1] - px[None, :]
    dy = xy[:, 1:2] - py[None, :]
    A_, B_, C_, op = co[:, 0:1], co[:, 1:2], co[:, 2:3], co[:, 3:4]
    # the forward, in float32 in its operation order (GSCuda.cu:634-657)
    dx32, dy32 = f(xy[:, 0:1]) - f(px[None, :]), f(xy[:, 1:2]) - f(py[None, :])
    A32, B32, C32, op32 = f(A_), f(B_), f(C_), f(op)
    power = f(-0.5) * ((A32 * dx32) * dx32 + (C32 * dy32) * dy32) - (B32 * dx32) * dy32
    G = cpu_oracle.expf(np.minimum(power, f(0.0))).reshape(power.shape)
    raw = op32 * G
    alpha = np.minimum(f(0.99), raw)
    valid = (power <= 0.0) & (alpha >= f(1.0 / 255.0)) & inside[None, :]
    a_eff = np.where(valid, alpha, f(0.0))
    t_after = np.cumprod(f(1.0) - a_eff, axis=0, dtype=np.float32).astype(np.float64)
    power, G, raw, alpha, a_eff = (v.astype(np.float64) for v in (power, G, raw, alpha, a_eff))
    t_before = np.vstack([np.ones((1, px.size)), t_after[:-1]])
    stop = valid & (t_after < t_cutoff)
    has_stop = stop.any(axis=0)
    stop_idx = np.where(has_stop, stop.argmax(axis=0), L)
    k = np.arange(L)[:, None]
    contrib = valid & (k < stop_idx[None, :])
    final_t = np.where(has_stop, t_before[np.minimum(stop_idx, L - 1), np.arange(px.size)], t_after[-1])
    w = np.where(contrib, alpha * t_before, 0.0)
    n_contrib = np.where(contrib.any(axis=0), L - np.argmax(contrib[::-1], axis=0), 0)
    # back to front: S_k = everything behind record k, dotted with the pixel's gradients; the opacity's term is its seed
    cg = chan @ gp
    wc = w * cg
    behind = (final_t * (bg @ gp - ga))[None, :] + (wc.sum(axis=0)[None, :] - np.cumsum(wc, axis=0))
    one_minus = 1.0 - np.where(contrib, alpha, 0.0)
    dL_dalpha = np.where(contrib, t_before * cg - behind / one_minus, 0.0)
    free = contrib & ~(raw > 0.99)
    dLp = op * G * np.where(free, dL_dalpha, 0.0)
    sx, sy = (-A_ * dx - B_ * dy) * dLp, (-C_ * dy - B_ * dx) * dLp          # the pixel's share of dL/d mean2D
    signed = np.stack([sx.sum(1), sy.sum(1)], 1)
    A = np.stack([np.abs(sx).sum(1), np.abs(sy).sum(1)], 1)
    ag = np.abs(gp)
    cga = np.abs(chan) @ ag
    behind_a = (final_t * (np.abs(bg) @ ag + np.abs(ga)))[None, :] + ((w * cga).sum(axis=0)[None, :] - np.cumsum(w * cga, axis=0))
    dLa_a = np.where(free, t_before * cga + behind_a / (1.0 - np.where(free, alpha, 0.0)), 0.0)
    dLp_a = op * G * dLa_a
    adx, ady = np.abs(dx), np.abs(dy)
    uxa, uya = np.abs(A_) * adx + np.abs(B_) * ady, np.abs(B_) * adx + np.abs(C_) * ady
    walk = np.cumsum(contrib[::-1], axis=0)[::-1]
    return {"signed": signed, "A": A, "M": np.stack([(uxa * dLp_a).sum(1), (uya * dLp_a).sum(1)], 1),
            "k": np.where(contrib, walk, 0).max(axis=1), "pixels": contrib.sum(axis=1), "free_pixels": free.sum(axis=1),
            "final_t": np.where(inside, final_t, 0.0).reshape(TILE, TILE), "n_contrib": n_contrib.reshape(TILE, TILE)}


def depth_values(means3D, view, inverse=False):
    """d_i as the blend computes it (blend_core.hpp: depth_value), float32 in its operation order."""
    f = np.float32
    m, v = np.asarray(means3D, f), np.asarray(view, f).reshape(-1)
    z = (v[2] * m[:, 0] + v[6] * m[:, 1]) + (v[10] * m[:, 2] + v[14] * f(1.0))
    with np.errstate(all="ignore"):
        return (f(1.0) / z).astype(f) if inverse else z.astype(f)


def frame_absgrad(state, width, height, background, g_color, g_depth=None, depths=None, g_alpha=None, t_cutoff=0.001,
                  tile_rows=None):
    """tile_absgrad over the tiles of rows `tile_rows` (default: all) of a forward state (means2D, conicOpacity, rgb, ranges,
    values: cpu_oracle.forward's dict or the GPU's arrays under those names), summed per Gaussian [N]. g_color [3,H,W];
    g_depth [H,W] with depths [N] (d_i: depth_values) adds the depth channel, over a zero background; g_alpha [H,W] the seed.
    Returns signed, A, M [N,2]; k, pixels, free_pixels [N]; final_t [H,W] (NaN outside the rows), n_contrib [H,W] (-1)."""
    means2D = np.asarray(state["means2D"], np.float32).reshape(-1, 2)
    conic = np.asarray(state["conicOpacity"], np.float32).reshape(-1, 4)
    chan = np.asarray(state["rgb"], np.float32).reshape(-1, 3)
    bg = np.asarray(background, np.float64)
    g = np.asarray(g_color, np.float64)
    if g_depth is not None:
        chan = np.concatenate([chan, np.asarray(depths, np.float32).reshape(-1, 1)], 1)
        bg = np.concatenate([bg, [0.0]])
        g = np.concatenate([g, np.asarray(g_depth, np.float64)[None]], 0)
    ranges = np.asarray(state["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    values = np.asarray(state["values"]).view(np.uint32).astype(np.int64)
    n, C = means2D.shape[0], chan.shape[1]
    gx, gy = (width + 15) // 16, (height + 15) // 16
    r0, r1 = (0, gy) if tile_rows is None else tile_rows
    out = {"signed": np.zeros((n, 2)), "A": np.zeros((n, 2)), "M": np.zeros((n, 2)), "k": np.zeros(n, np.int64),
           "pixels": np.zeros(n, np.int64), "free_pixels": np.zeros(n, np.int64),
           "final_t": np.full((height, width), np.nan), "n_contrib": np.full((height, width), -1, np.int64)}
    for ty in range(r0, r1):
        for tx in range(gx):
            a, b = (int(v) for v in ranges[ty * gx + tx])
            ids = values[a:b] if b > a else values[0:0]
            ya, yb, xa, xb = ty * 16, min(height, ty * 16 + 16), tx * 16, min(width, tx * 16 + 16)
            tile_g = np.zeros((C, 16, 16))
            tile_g[:, : yb - ya, : xb - xa] = g[:, ya:yb, xa:xb]
            tile_a = None
            if g_alpha is not None:
                tile_a = np.zeros((16, 16))
                tile_a[: yb - ya, : xb - xa] = np.asarray(g_alpha, np.float64)[ya:yb, xa:xb]
            res = tile_absgrad(means2D[ids], conic[ids], chan[ids], tx, ty, width, height, bg, tile_g, tile_a, t_cutoff)
            for key in ("signed", "A", "M", "pixels", "free_pixels"):
                np.add.at(out[key], ids, res[key])
            np.maximum.at(out["k"], ids, res["k"])
            out["final_t"][ya:yb, xa:xb] = res["final_t"][: yb - ya, : xb - xa]
            out["n_contrib"][ya:yb, xa:xb] = res["n_contrib"][: yb - ya, : xb - xa]
    return out


def bound(ref):
    """helpers.py's rule of the render backward, unchanged: BW_TAU (k + BW_C) M + BW_ATOL, per Gaussian and component."""
    from helpers import BW_ATOL, BW_C, BW_TAU
    return BW_TAU * (ref["k"].astype(np.float64) + BW_C)[:, None] * ref["M"] + BW_ATOL


# ---- scenes and pixel gradients ---------------------------------------------------------------------------------------------
LIST_LENGTHS = (1, 63, 64, 65, 255, 256, 257)        # the wave's batch of 64 and the reference's round of 256


@functools.lru_cache(maxsize=None)
def clamp_scene():
    """40 x 24 (partial right and bottom tiles): 60 ordinary, rather faint splats in front of 24 wide ones whose opacity is 0.9995
    to 0.99999 — raw > 0.99 within about 0.14 sigma of their centres, below it further out — so that records are clamped on
    some of the pixels that blend them and free on the others (the callers assert how many)."""
    import contrib_ref as R
    cam = R._camera(40, 24)
    rng = np.random.default_rng(91)
    wide = R._rows(rng, 24, (0, 1), (0, 1), (1.0, 2.0), (5.0, 8.0), (0.9995, 0.99999))
    wide[:, 0], wide[:, 1] = 3.0 + 6.0 * (np.arange(24) % 6), 3.0 + 6.0 * (np.arange(24) // 6)      # a 6 x 4 grid, on pixel centres
    rows = np.concatenate([wide,
                           R._rows(rng, 60, (0, 40), (0, 24), (-1.0, 0.9), (0.5, 3.0), (0.01, 0.4)),
                           R._rows(rng, 4, (-300, -250), (0, 24), (-1.0, 1.0), (0.5, 1.0), (0.5, 0.9))])
    return R._splats(cam, rows), cam


def all_scenes():
    """(name, scene, camera) of every scene the GPU file compares with the reference."""
    import contrib_ref as R
    for length in LIST_LENGTHS:
        for opaque in (False, True):
            scene, cam = R.one_tile_scene(length, opaque)
            yield f"tile-{length}-{'opaque' if opaque else 'faint'}", scene, cam
    yield ("edge",) + R.edge_scene()         # 40 x 24: partial right and bottom tiles, faint records, opaque stacks
    yield ("fill",) + R.fill_scene()         # 128 x 128: one splat over 64 tiles
    yield ("clamp",) + clamp_scene()


BACKGROUND = (0.3, -0.2, 0.5)


def pixel_gradients(cam, seed=5):
    """(g_color [3,H,W], g_depth [H,W], g_alpha [H,W]) float32, standard normal: of either sign within every splat, so that a
    splat's signed sum cancels where its absolute sum does not."""
    rng = np.random.default_rng(seed + 1000 * cam.width + cam.height)
    f = np.float32
    return (rng.normal(size=(3, cam.height, cam.width)).astype(f), rng.normal(size=(cam.height, cam.width)).astype(f),
            rng.normal(size=(cam.height, cam.width)).astype(f))


TERMS = ("colour", "colour+depth", "colour+inverse", "colour+alpha", "all")


def reference(state, scene, cam, terms, semantics="gscuda", tile_rows=None, seed=5):
    """frame_absgrad of `state` for one of TERMS with pixel_gradients(cam, seed) over BACKGROUND."""
    gc, gd, ga = pixel_gradients(cam, seed)
    depth = terms in ("colour+depth", "colour+inverse", "all")
    d = depth_values(scene["means3D"], cam.view, inverse=terms == "colour+inverse") if depth else None
    return frame_absgrad(state, cam.width, cam.height, BACKGROUND, gc, gd if depth else None, d,
                         ga if terms in ("colour+alpha", "all") else None, T_CUTOFF[semantics], tile_rows)
