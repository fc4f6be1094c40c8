"""Reference of the N-channel feature maps (include/gsrast_amd_features.h), shared by tests/test_features_cpu.py and
tests/test_gpu_features.py with the scenes, features and pixel gradients both files use.

Forward: a float32 replay in the blend's operation order — the masks, the power, exp = the C++ oracle's libm expf, alpha and
T = T (1 - alpha) as tests/contrib_ref.contribution replays them, the cut-off test included (so finalT / nContrib of the replay are
the forward call's, which the callers assert) — that keeps acc[c] = fmaf(f[c], alpha T, acc[c]) per channel, the fused
multiply-add rounded ONCE (fma32), and leaves out = acc + finalT * bg as two float32 operations.
Backward: a float64 walk over the float32 decisions, tests/absgrad_ref.tile_absgrad generalised: C channels, the signed sums of
every geometry slot (mean2D, conic, opacity, cov2D) and of the channels, each with its condition scale M (every factor replaced
by its absolute value) and the walk depth k, as oracle/backward_np.blend_tile_backward defines them for three channels."""
import numpy as np

import absgrad_ref as A
import contrib_ref

F = np.float32
TILE = 16
T_CUTOFF = contrib_ref.T_CUTOFF
CHUNK, NARROW = 16, 8                       # GSR_FEATURES_CHUNK, GSR_FEATURES_CHUNK_NARROW (tests/test_features_cpu.py holds them against the header)
# 1, 3; around the width at which a call changes from the narrow kernels to the wide ones; K - 1, K, K + 1, 2 K + 1 of the wide ones
CHANNELS = (1, 3, NARROW - 1, NARROW, NARROW + 1, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
SUMS = (("d_mean", 2), ("d_conic", 3), ("d_op", 1), ("d_cov", 3))      # the geometry sums, in the order of sums_f64's slots 0..5, 9..11


def fma32(a, b, c):
    """float32 fused multiply-add, correctly rounded: the product of two float32 is exact in float64; the sum is rounded to odd
    there (TwoSum gives the error's sign), and 53 bits rounded to odd round to the 24-bit result of the exact sum."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    p, c = np.broadcast_arrays(p, c)
    with np.errstate(all="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0.0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(F)


def _pixels(tx, ty, W, H):
    ly, lx = np.divmod(np.arange(256), 16)
    px, py = tx * 16 + lx, ty * 16 + ly
    return px, py, (px < W) & (py < H)


def forward(state, features, background, W, H, t_cutoff=0.001, tile_rows=None, fused=True):
    """out [C,H,W] float32 (NaN on the rows outside `tile_rows`), finalT [H,W], nContrib [H,W] of the replay over a forward state
    (means2D, conicOpacity, ranges, values: cpu_oracle.forward's dict or the GPU's arrays). background: [C] or None.
    fused=False: the sums as the reference's loop forms them instead, acc + (f * alpha) * T in three roundings (GSCuda.cu:657) —
    what oracle/oracle_np.py and the C++ oracle compute, bit for bit; the walk, alpha, T and the decisions are the same."""
    means2D = np.asarray(state["means2D"], F).reshape(-1, 2)
    co = np.asarray(state["conicOpacity"], F).reshape(-1, 4)
    ranges = np.asarray(state["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    values = np.asarray(state["values"]).view(np.uint32).astype(np.int64)
    feat = np.asarray(features, F)
    C = feat.shape[1]
    bg = None if background is None else np.asarray(background, F).reshape(C)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r0_, r1_ = (0, gy) if tile_rows is None else tile_rows
    out, sums = np.full((C, H, W), np.nan, F), np.full((C, H, W), np.nan, F)
    finalT, ncontrib = np.zeros((H, W), F), np.zeros((H, W), np.uint32)
    exp = contrib_ref._libm_exp
    with np.errstate(all="ignore"):
        for ty in range(r0_, r1_):
            for tx in range(gx):
                r0, r1 = (int(v) for v in ranges[ty * gx + tx])
                px, py, inside = _pixels(tx, ty, W, H)
                fx, fy = px.astype(F), py.astype(F)
                done = ~inside
                T = np.ones(256, F)
                acc = np.zeros((C, 256), F)
                contrib, last = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
                for k in range(r0, max(r0, r1)):
                    if done.all():
                        break
                    g = int(values[k])
                    act = ~done
                    contrib[act] += 1
                    gxy, con = means2D[g], co[g]
                    dx, dy = gxy[0] - fx, gxy[1] - fy
                    power = F(-0.5) * (con[0] * dx * dx + con[2] * dy * dy) - con[1] * dx * dy
                    alpha = np.minimum(F(0.99), con[3] * exp(power))
                    test = T * (F(1.0) - alpha)
                    live = act & ~(power > 0) & ~(alpha < F(1.0) / F(255.0))
                    stop = live & (test < F(t_cutoff))
                    upd = live & ~stop
                    done |= stop
                    if upd.any() and fused:
                        w = (alpha * T).astype(F)
                        acc[:, upd] = fma32(feat[g][:, None], w[None, upd], acc[:, upd])
                    elif upd.any():
                        acc[:, upd] = acc[:, upd] + (feat[g][:, None] * alpha[None, upd]) * T[None, upd]
                    T[upd] = test[upd]
                    last[upd] = contrib[upd]
                ys, xs = py[inside], px[inside]
                res = acc if bg is None else (acc + (T[None, :] * bg[:, None]).astype(F)).astype(F)
                out[:, ys, xs] = res[:, inside]
                sums[:, ys, xs] = acc[:, inside]
                finalT[ys, xs] = T[inside]
                ncontrib[ys, xs] = last[inside]
    return {"out": out, "acc": sums, "finalT": finalT, "nContrib": ncontrib}     # (acc: the sums alone, `out` of a NULL background)


def tile_backward(xy, co, chan, tx, ty, width, height, background, g_tile, t_cutoff=0.001, f32_forward=True):
    """One 16 x 16 tile, [L records x 256 pixels], float64 sums over the float32 forward (blend_tile_backward's f32_forward
    semantics; f32_forward=False: the forward in float64 too, the function finite differences can be taken of).
    chan [L,C], background [C], g_tile [C,16,16]. Returns per record d_mean [L,2], d_conic [L,3], d_op [L,1],
    d_cov [L,3], d_chan [L,C], "M_" + each (the condition scales), k, pixels, free_pixels [L]; out [C,16,16] (float64 blend over
    the float32 weights), final_t, n_contrib [16,16]."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    co = np.asarray(co, np.float64).reshape(-1, 4)
    L = xy.shape[0]
    chan = np.asarray(chan, np.float64).reshape(L, -1)
    C = chan.shape[1]
    bg = np.zeros(C) if background is None else np.asarray(background, np.float64).reshape(C)
    ys, xs = np.mgrid[0:TILE, 0:TILE]
    px = (tx * TILE + xs).reshape(-1).astype(np.float64)
    py = (ty * TILE + ys).reshape(-1).astype(np.float64)
    inside = (px < width) & (py < height)
    gp = np.asarray(g_tile, np.float64).reshape(C, -1) * inside[None, :]
    if L == 0:
        res = {name: np.zeros((0, d)) for name, d in SUMS + (("d_chan", C),)}
        res.update({"M_" + name: np.zeros((0, d)) for name, d in SUMS + (("d_chan", C),)})
        zi = np.zeros(0, np.int64)
        res.update(k=zi, pixels=zi.copy(), free_pixels=zi.copy(), out=np.where(inside[None, :], bg[:, None], 0.0).reshape(C, TILE, TILE),
                   final_t=inside.astype(np.float64).reshape(TILE, TILE), n_contrib=np.zeros((TILE, TILE), np.int64))
        return res
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
    if not f32_forward:
        power = -0.5 * (A_ * dx * dx + C_ * dy * dy) - B_ * dx * dy
        G = np.exp(np.minimum(power, 0.0))
        raw = op * G
        alpha = np.minimum(0.99, raw)
        valid = (power <= 0.0) & (alpha >= 1.0 / 255.0) & inside[None, :]
        t_after = np.cumprod(1.0 - np.where(valid, alpha, 0.0), axis=0)
    t_before = np.vstack([np.ones((1, px.size)), t_after[:-1]])
    stop = valid & (t_after < t_cutoff)
    has_stop = stop.any(axis=0)
    stop_idx = np.where(has_stop, stop.argmax(axis=0), L)
    k = np.arange(L)[:, None]
    contrib = valid & (k < stop_idx[None, :])
    final_t = np.where(has_stop, t_before[np.minimum(stop_idx, L - 1), np.arange(px.size)], t_after[-1])
    w = np.where(contrib, alpha * t_before, 0.0)
    out = chan.T @ w + final_t[None, :] * bg[:, None]
    n_contrib = np.where(contrib.any(axis=0), L - np.argmax(contrib[::-1], axis=0), 0)
    # back to front: S_k = everything behind record k, dotted with the pixel's gradients
    cg = chan @ gp
    wc = w * cg
    behind = (final_t * (bg @ gp))[None, :] + (wc.sum(axis=0)[None, :] - np.cumsum(wc, axis=0))
    dL_dalpha = np.where(contrib, t_before * cg - behind / (1.0 - np.where(contrib, alpha, 0.0)), 0.0)
    free = contrib & ~(raw > 0.99)
    dLa = np.where(free, dL_dalpha, 0.0)
    dLp = op * G * dLa
    ux, uy = A_ * dx + B_ * dy, B_ * dx + C_ * dy
    res = {"d_chan": w @ gp.T,
           "d_op": (G * dLa).sum(axis=1)[:, None],
           "d_conic": np.stack([(-0.5 * dx * dx * dLp).sum(1), (-dx * dy * dLp).sum(1), (-0.5 * dy * dy * dLp).sum(1)], 1),
           "d_mean": np.stack([(-ux * dLp).sum(1), (-uy * dLp).sum(1)], 1),
           "d_cov": np.stack([(0.5 * ux * ux * dLp).sum(1), (0.5 * ux * uy * dLp).sum(1), (0.5 * uy * uy * dLp).sum(1)], 1)}
    ag = np.abs(gp)
    cga = np.abs(chan) @ ag
    behind_a = (final_t * (np.abs(bg) @ ag))[None, :] + ((w * cga).sum(axis=0)[None, :] - np.cumsum(w * cga, axis=0))
    dLa_a = np.where(free, t_before * cga + behind_a / (1.0 - np.where(free, alpha, 0.0)), 0.0)
    dLp_a = op * G * dLa_a
    adx, ady = np.abs(dx), np.abs(dy)
    uxa, uya = np.abs(A_) * adx + np.abs(B_) * ady, np.abs(B_) * adx + np.abs(C_) * ady
    walk = np.cumsum(contrib[::-1], axis=0)[::-1]
    res.update(M_d_chan=w @ ag.T, M_d_op=(G * dLa_a).sum(axis=1)[:, None],
               M_d_conic=np.stack([(0.5 * adx * adx * dLp_a).sum(1), (adx * ady * dLp_a).sum(1), (0.5 * ady * ady * dLp_a).sum(1)], 1),
               M_d_mean=np.stack([(uxa * dLp_a).sum(1), (uya * dLp_a).sum(1)], 1),
               M_d_cov=np.stack([(0.5 * uxa * uxa * dLp_a).sum(1), (0.5 * uxa * uya * dLp_a).sum(1), (0.5 * uya * uya * dLp_a).sum(1)], 1),
               k=np.where(contrib, walk, 0).max(axis=1), pixels=contrib.sum(axis=1), free_pixels=free.sum(axis=1),
               out=np.where(inside[None, :], out, 0.0).reshape(C, TILE, TILE),
               final_t=np.where(inside, final_t, 0.0).reshape(TILE, TILE), n_contrib=n_contrib.reshape(TILE, TILE))
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
    means2D = np.asarray(state["means2D"], np.float32).reshape(-1, 2)
    conic = np.asarray(state["conicOpacity"], np.float32).reshape(-1, 4)
    chan = np.asarray(features)
    chan = chan.astype(np.float32) if chan.dtype != np.float64 else chan
    n, C = chan.shape
    g = np.asarray(g, np.float64).reshape(C, H, W)
    ranges = np.asarray(state["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    values = np.asarray(state["values"]).view(np.uint32).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r0, r1 = (0, gy) if tile_rows is None else tile_rows
    names = [name for name, _ in SUMS] + ["d_chan"]
    dims = dict(SUMS + (("d_chan", C),))
    out = {name: np.zeros((n, dims[name])) for name in names}
    out.update({"M_" + name: np.zeros((n, dims[name])) for name in names})
    out.update(k=np.zeros(n, np.int64), pixels=np.zeros(n, np.int64), free_pixels=np.zeros(n, np.int64), tiles=np.zeros(n, np.int64),
               final_t=np.full((H, W), np.nan), n_contrib=np.full((H, W), -1, np.int64))
    for ty in range(r0, r1):
        for tx in range(gx):
            a, b = (int(v) for v in ranges[ty * gx + tx])
            ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
            if prefix and b > a:
                b = min(b, a + int(np.asarray(state["nContrib"]).view(np.uint32).reshape(H, W)[ya:yb, xa:xb].max()))
            ids = values[a:b] if b > a else values[0:0]
            tile_g = np.zeros((C, 16, 16))
            tile_g[:, : yb - ya, : xb - xa] = g[:, ya:yb, xa:xb]
            res = tile_backward(means2D[ids], conic[ids], chan[ids], tx, ty, W, H, background, tile_g, t_cutoff)
            for name in names:
                np.add.at(out[name], ids, res[name])
                np.add.at(out["M_" + name], ids, res["M_" + name])
            for key in ("pixels", "free_pixels"):
                np.add.at(out[key], ids, res[key])
            np.maximum.at(out["k"], ids, res["k"])
            np.add.at(out["tiles"], ids, (res["pixels"] > 0).astype(np.int64))
            out["final_t"][ya:yb, xa:xb] = res["final_t"][: yb - ya, : xb - xa]
            out["n_contrib"][ya:yb, xa:xb] = res["n_contrib"][: yb - ya, : xb - xa]
    return out


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
