"""Reference of the N-channel feature maps (include/gsrast_amd_features.h), shared by tests/test_features_cpu.py and
tests/test_gpu_features.py with the scenes, features and pixel gradients both files use.

Forward: a float32 replay in the blend's operation order — the masks, the power, exp = the C++ oracle's libm expf, alpha and
T = T (1 - alpha) as tests/walk_ref.replay holds them, the cut-off test included (so finalT / nContrib of the replay are
the forward call's, which the callers assert) — that keeps acc[c] = fmaf(f[c], alpha T, acc[c]) per channel, the fused
multiply-add rounded ONCE (fma32), and leaves out = acc + finalT * bg as two float32 operations.
Backward: a float64 walk over the float32 decisions (walk_ref.tile_decisions, geometry_sums and frame): C channels, the signed sums of
every geometry slot (mean2D, conic, opacity, cov2D) and of the channels, each with its condition scale M (every factor replaced
by its absolute value) and the walk depth k, as oracle/backward_np.blend_tile_backward defines them for three channels."""
import numpy as np

import absgrad_ref as A
import walk_ref
from walk_ref import T_CUTOFF, TILE, fma32      # noqa: F401  (T_CUTOFF: a name the callers take from here)

F = np.float32
CHUNK, NARROW = 16, 8                       # GSR_FEATURES_CHUNK, GSR_FEATURES_CHUNK_NARROW (tests/test_features_cpu.py holds them against the header)
# 1, 3; around the width at which a call changes from the narrow kernels to the wide ones; K - 1, K, K + 1, 2 K + 1 of the wide ones
CHANNELS = (1, 3, NARROW - 1, NARROW, NARROW + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SUMS = walk_ref.GEOMETRY


def forward(state, features, background, W, H, t_cutoff=0.001, tile_rows=None, fused=True):
    """out [C,H,W] float32 (NaN on the rows outside `tile_rows`), finalT [H,W], nContrib [H,W] of the replay over a forward state
    (means2D, conicOpacity, ranges, values: cpu_oracle.forward's dict or the GPU's arrays). background: [C] or None.
    fused=False: the sums as the reference's loop forms them instead, acc + (f * alpha) * T in three roundings (GSCuda.cu:657) —
    what oracle/oracle_np.py and the C++ oracle compute, bit for bit; the walk, alpha, T and the decisions are the same."""
    feat = np.asarray(features, F)
    C = feat.shape[1]
    bg = None if background is None else np.asarray(background, F).reshape(C)
    out, sums = np.full((C, H, W), np.nan, F), np.full((C, H, W), np.nan, F)

    def start(tx, ty):
        return np.zeros((C, 256), F)

    def record(acc, g, pos, con, dx, dy, power, alpha, T, upd):
        if fused:
            w = (alpha * T).astype(F)
            acc[:, upd] = fma32(feat[g][:, None], w[None, upd], acc[:, upd])
        else:
            acc[:, upd] = acc[:, upd] + (feat[g][:, None] * alpha[None, upd]) * T[None, upd]

    def end(acc, px, py, inside, T, last, done):
        ys, xs = py[inside], px[inside]
        res = acc if bg is None else (acc + (T[None, :] * bg[:, None]).astype(F)).astype(F)
        out[:, ys, xs] = res[:, inside]
        sums[:, ys, xs] = acc[:, inside]

    finalT, ncontrib, _ = walk_ref.replay(state["means2D"], state["conicOpacity"], state["ranges"], state["values"], W, H, t_cutoff,
                                          tile_rows, None, start, record, end)
    return {"out": out, "acc": sums, "finalT": finalT, "nContrib": ncontrib}     # (acc: the sums alone, `out` of a NULL background)


def tile_backward(xy, co, chan, tx, ty, width, height, background, g_tile, t_cutoff=0.001, f32_forward=True):
    """One 16 x 16 tile, [L records x 256 pixels], float64 sums over the float32 forward (blend_tile_backward's f32_forward
    semantics; f32_forward=False: the forward in float64 too, the function finite differences can be taken of).
    chan [L,C], background [C], g_tile [C,16,16]. Returns per record d_mean [L,2], d_conic [L,3], d_op [L,1],
    d_cov [L,3], d_chan [L,C], "M_" + each (the condition scales), k, pixels, free_pixels [L]; out [C,16,16] (float64 blend over
    the float32 weights), final_t, n_contrib [16,16]."""
    d = walk_ref.tile_decisions(xy, co, tx, ty, width, height, t_cutoff, f32_forward)
    chan = np.asarray(chan, np.float64).reshape(d.L, -1)
    C = chan.shape[1]
    bg = np.zeros(C) if background is None else np.asarray(background, np.float64).reshape(C)
    inside = d.inside
    if d.L == 0:
        return walk_ref.empty_tile(d, walk_ref.with_scales(SUMS + (("d_chan", C),)), "k",
                                   out=np.where(inside[None, :], bg[:, None], 0.0).reshape(C, TILE, TILE))
    gp = np.asarray(g_tile, np.float64).reshape(C, -1) * inside[None, :]
    w, final_t, t_before, alpha, contrib, free = d.w, d.final_t, d.t_before, d.alpha, d.contrib, d.free
    out = chan.T @ w + final_t[None, :] * bg[:, None]
    # back to front: S_k = everything behind record k, dotted with the pixel's gradients
    cg = chan @ gp
    wc = w * cg
    behind = (final_t * (bg @ gp))[None, :] + (wc.sum(axis=0)[None, :] - np.cumsum(wc, axis=0))
    dL_dalpha = np.where(contrib, t_before * cg - behind / (1.0 - np.where(contrib, alpha, 0.0)), 0.0)
    ag = np.abs(gp)
    cga = np.abs(chan) @ ag
    behind_a = (final_t * (np.abs(bg) @ ag))[None, :] + ((w * cga).sum(axis=0)[None, :] - np.cumsum(w * cga, axis=0))
    dLa_a = np.where(free, t_before * cga + behind_a / (1.0 - np.where(free, alpha, 0.0)), 0.0)
    res = walk_ref.geometry_sums(d, dL_dalpha, dLa_a)
    res.update(walk_ref.tile_maps(d), d_chan=w @ gp.T, M_d_chan=w @ ag.T, k=d.k, out=np.where(inside[None, :], out, 0.0).reshape(C, TILE, TILE))
    return res


def joint_channels(rgb, background, g_color, features=None, g_features=None, depths=None, g_depth=None, g_alpha=None):
    """(chan [N,C'], bg [C'], g [C',H,W]) of ONE backward() call with every term, as channels of the walk: the colours over
    `background`, d_i over zero, the accumulated opacity as a channel that is 0 on every Gaussian over a background of -1 (its
    whole term is the seed -T_f g_a), the features over zero. Columns: 0..2 colour, then depth, alpha, features as given."""
    n = rgb.shape[0]
    chan, bg, g = [np.asarray(rgb, np.float64)], [np.asarray(background, np.float64)], [np.asarray(g_color, np.float64)]
    if g_depth is not None:
        chan.append(np.asarray(depths, np.float64).reshape(n, 1)); bg.append(np.zeros(1)); g.append(np.asarray(g_depth, np.float64)[None])
    if g_alpha is not None:
        chan.append(np.zeros((n, 1))); bg.append(-np.ones(1)); g.append(np.asarray(g_alpha, np.float64)[None])
    if features is not None:
        chan.append(np.asarray(features, np.float64)); bg.append(np.zeros(features.shape[1])); g.append(np.asarray(g_features, np.float64))
    return np.concatenate(chan, 1), np.concatenate(bg), np.concatenate(g, 0)


def backward(state, features, background, g, W, H, t_cutoff=0.001, tile_rows=None, prefix=False):
    """tile_backward over the tiles of rows `tile_rows` (default: all) of a forward state, summed per Gaussian: d_* and M_d_* [N,.],
    k, pixels, free_pixels, tiles [N] (tiles: where some pixel blended it), final_t [H,W] (NaN outside the rows), n_contrib [H,W]
    (-1 there). g [C,H,W]. prefix: walk each tile's list only as far as state["nContrib"] reaches (the caller compares n_contrib)."""
    chan = np.asarray(features)
    chan = chan.astype(np.float32) if chan.dtype != np.float64 else chan
    C = chan.shape[1]

    def tile(xy, co, ids, tx, ty, g):
        return tile_backward(xy, co, chan[ids], tx, ty, W, H, background, g, t_cutoff)

    return walk_ref.frame(state, W, H, tile_rows, {"g": np.asarray(g, np.float64).reshape(C, H, W)}, tile,
                          walk_ref.with_scales(SUMS + (("d_chan", C),)), "k", tiles=True, prefix=prefix)


def bound(ref, name, float_tile_sums=False):
    """helpers.py's rule of the render backward, unchanged: BW_TAU (k + BW_C [+ tiles]) M + BW_ATOL, per Gaussian and component
    (float_tile_sums, a bool or bool[N]: the Gaussian's sums passed through the block feed's per-entry floats)."""
    from helpers import BW_ATOL, BW_C, BW_TAU
    depth = ref["k"].astype(np.float64) + BW_C + np.where(np.asarray(float_tile_sums, bool), ref["tiles"].astype(np.float64), 0.0)
    return BW_TAU * depth[:, None] * ref["M_" + name] + BW_ATOL


def worst_ratio(got, ref, name):
    """max |got - ref| / ((k + BW_C) M) over the components with M > 0."""
    from helpers import BW_C
    err = np.abs(np.asarray(got, np.float64) - ref[name])
    scale = (ref["k"].astype(np.float64) + BW_C)[:, None] * ref["M_" + name]
    ratio = np.where(ref["M_" + name] > 0, err / np.maximum(scale, 1e-300), 0.0)
    return float(ratio.max()) if ratio.size else 0.0


# ---- scenes, features and pixel gradients -----------------------------------------------------------------------------------
LIST_LENGTHS = A.LIST_LENGTHS
BACKGROUND = A.BACKGROUND


def all_scenes():
    """(name, scene, camera): contrib_ref.one_tile_scene at every list length, faint and opaque; edge; fill; absgrad_ref.clamp_scene."""
    return A.all_scenes()


def features_of(n, channels, seed=11):
    """[n, channels] float32, standard normal: of either sign, no channel like another."""
    return np.random.default_rng(seed + 7919 * channels + n).normal(size=(n, channels)).astype(F)


def background_of(channels, seed=13):
    return np.random.default_rng(seed + channels).uniform(-1.0, 1.0, channels).astype(F)


def gradient_of(cam, channels, seed=17):
    """[channels, H, W] float32, standard normal."""
    return np.random.default_rng(seed + 31 * channels + 1000 * cam.width + cam.height).normal(size=(channels, cam.height, cam.width)).astype(F)


def colours_of(scene):
    """The colours the gscuda profile composites, 0.5 + 0.4 DC in float32 (GSCuda.cu:362-366)."""
    dc = np.asarray(scene["shs"], F)[:, :3]
    return (F(0.5) + F(0.4) * dc).astype(F)
