"""Reference of the absolute screen-space gradient (include/gsrast_amd_absgrad.h): float64, tile-vectorised [L records x 256
pixels] the way oracle/backward_np.blend_tile_backward is, over the forward's float32 decisions (its f32_forward=True semantics:
power, exp = libm's expf, alpha and the transmittance product in float32 in the forward's operation order; the sums in float64).
It takes C channels — (r, g, b) or (r, g, b, d) — with a pixel gradient per channel, a background per channel and an optional
seed for the accumulated opacity, so that the three terms of L enter one dL/dalpha per pixel as they do in the kernel.
The decisions, the geometry sums and the frame driver are tests/walk_ref.py's; here stand `behind` with the opacity seed.
Shared by tests/test_absgrad_cpu.py and tests/test_gpu_absgrad.py, with the scenes and the pixel gradients both files use."""
import functools

import numpy as np

import walk_ref
from walk_ref import T_CUTOFF, TILE, depth_values      # noqa: F401  (TILE: a public name of this module)


def tile_absgrad(xy, co, chan, tx, ty, width, height, background, g_tile, g_alpha_tile=None, t_cutoff=0.001):
    """One 16 x 16 tile. xy [L,2], co [L,4], chan [L,C]: the records of the tile's list, front to back; background [C];
    g_tile [C,16,16] and g_alpha_tile [16,16] or None (entries outside the image are ignored).
    Returns per record: signed [L,2] (the render backward's d_mean), A [L,2] (the sum over pixels of |share|), M [L,2] (the
    condition scale: the same sum with every factor replaced by its absolute value — dL/dalpha becomes |T_before cg| +
    |behind / (1 - alpha)|, cg and `behind` themselves sums of absolute values, the opacity seed entering as |g_a|), k [L] (the
    walk depth), pixels / free_pixels [L]; per pixel final_t, n_contrib [16,16]."""
    d = walk_ref.tile_decisions(xy, co, tx, ty, width, height, t_cutoff)
    chan = np.asarray(chan, np.float64)
    chan = chan.reshape(d.L, -1)
    bg = np.asarray(background, np.float64)
    C = chan.shape[1]
    assert bg.shape == (C,), (bg.shape, C)
    if d.L == 0:
        return walk_ref.empty_tile(d, (("signed", 2), ("A", 2), ("M", 2)), "k")
    inside = d.inside
    gp = np.asarray(g_tile, np.float64).reshape(C, -1) * inside[None, :]
    ga = np.zeros(inside.size) if g_alpha_tile is None else np.asarray(g_alpha_tile, np.float64).reshape(-1) * inside
    w, final_t, t_before, alpha, contrib, free = d.w, d.final_t, d.t_before, d.alpha, d.contrib, d.free
    # back to front: S_k = everything behind record k, dotted with the pixel's gradients; the opacity's term is its seed
    cg = chan @ gp
    wc = w * cg
    behind = (final_t * (bg @ gp - ga))[None, :] + (wc.sum(axis=0)[None, :] - np.cumsum(wc, axis=0))
    dL_dalpha = np.where(contrib, t_before * cg - behind / (1.0 - np.where(contrib, alpha, 0.0)), 0.0)
    ag = np.abs(gp)
    cga = np.abs(chan) @ ag
    behind_a = (final_t * (np.abs(bg) @ ag + np.abs(ga)))[None, :] + ((w * cga).sum(axis=0)[None, :] - np.cumsum(w * cga, axis=0))
    dLa_a = np.where(free, t_before * cga + behind_a / (1.0 - np.where(free, alpha, 0.0)), 0.0)
    geo = walk_ref.geometry_sums(d, dL_dalpha, dLa_a, shares=True)
    return dict(walk_ref.tile_maps(d), signed=geo["d_mean"], A=geo["A_d_mean"], M=geo["M_d_mean"], k=d.k)


def frame_absgrad(state, width, height, background, g_color, g_depth=None, depths=None, g_alpha=None, t_cutoff=0.001,
                  tile_rows=None):
    """tile_absgrad over the tiles of rows `tile_rows` (default: all) of a forward state (means2D, conicOpacity, rgb, ranges,
    values: cpu_oracle.forward's dict or the GPU's arrays under those names), summed per Gaussian [N]. g_color [3,H,W];
    g_depth [H,W] with depths [N] (d_i: depth_values) adds the depth channel, over a zero background; g_alpha [H,W] the seed.
    Returns signed, A, M [N,2]; k, pixels, free_pixels [N]; final_t [H,W] (NaN outside the rows), n_contrib [H,W] (-1)."""
    chan = np.asarray(state["rgb"], np.float32).reshape(-1, 3)
    bg = np.asarray(background, np.float64)
    g = np.asarray(g_color, np.float64)
    if g_depth is not None:
        chan = np.concatenate([chan, np.asarray(depths, np.float32).reshape(-1, 1)], 1)
        bg = np.concatenate([bg, [0.0]])
        g = np.concatenate([g, np.asarray(g_depth, np.float64)[None]], 0)

    def tile(xy, co, ids, tx, ty, g, g_alpha):
        return tile_absgrad(xy, co, chan[ids], tx, ty, width, height, bg, g, g_alpha, t_cutoff)

    return walk_ref.frame(state, width, height, tile_rows, {"g": g, "g_alpha": None if g_alpha is None else np.asarray(g_alpha, np.float64)},
                          tile, (("signed", 2), ("A", 2), ("M", 2)), "k")


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
