"""Reference of the depth distortion map (include/gsrast_amd_distortion.h), shared by tests/test_distortion_cpu.py and
tests/test_gpu_distortion.py with the scenes (absgrad_ref.all_scenes, imported), the values and the pixel gradients both use.

forward32: the float32 restatement of the header's forward, line for line, in features_ref.forward's replay (the masks, the
power, exp = libm's expf, alpha, the cut-off) with every fmaf rounded once (features_ref.fma32). The GPU's out and moments are
compared with it bit for bit.
tile_walk: a float64 walk, forward and backward, over the float32 forward's decisions (features_ref.tile_backward's: power,
exp, alpha and the transmittance product in float32), handed the float32 moments m0, M1n, M2n the kernel reads — the header's
formulas in exact arithmetic on the kernel's own inputs. Per record it returns every sum, its condition scale M — the same sum
with every factor and every subtraction taken in absolute value: 1 - T counts as 1 + T, T_{i+1} - T_f as their sum, c as the sum
of its summands' magnitudes — and n, the largest number of records blended into any pixel that blended the record.
Acceptance is helpers.py's rule with n in place of k (each term uses totals over the pixel's whole list, not over the records
behind it):  |got - exp| <= BW_TAU (n + BW_C) M + BW_ATOL."""
import numpy as np

import absgrad_ref as A
import contrib_ref
import features_ref as FR

F = np.float32
TILE = 16
T_CUTOFF = contrib_ref.T_CUTOFF
POWERS = (2, 1)
SUMS = FR.SUMS + (("d_val", 1),)
fma32 = FR.fma32


def all_scenes():
    return A.all_scenes()


def depth_values(scene, cam):
    """The scene's view depth, float32 (absgrad_ref.depth_values)."""
    return A.depth_values(scene["means3D"], cam.view)


def random_values(n, seed=29):
    """[n] float32, standard normal: of either sign, in no order along the lists."""
    return np.random.default_rng(seed + n).normal(size=n).astype(F)


def gradient_of(cam, seed=37):
    """[H, W] float32, standard normal."""
    return np.random.default_rng(seed + 1000 * cam.width + cam.height).normal(size=(cam.height, cam.width)).astype(F)


# ---- the float32 forward ------------------------------------------------------------------------------------------------------
def forward32(state, values, power, W, H, t_cutoff=0.001, tile_rows=None):
    """out [H,W], moments [3,H,W] float32 (NaN on the rows outside `tile_rows`), finalT [H,W], nContrib [H,W], blended [H,W]
    (how many records each pixel blended) of the replay over a forward state (means2D, conicOpacity, ranges, values)."""
    assert power in (1, 2)
    means2D = np.asarray(state["means2D"], F).reshape(-1, 2)
    co = np.asarray(state["conicOpacity"], F).reshape(-1, 4)
    ranges = np.asarray(state["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    lists = np.asarray(state["values"]).view(np.uint32).astype(np.int64)
    val = np.asarray(values, F).reshape(-1)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r0_, r1_ = (0, gy) if tile_rows is None else tile_rows
    out, mom = np.full((H, W), np.nan, F), np.full((3, H, W), np.nan, F)
    finalT, ncontrib, blended = np.zeros((H, W), F), np.zeros((H, W), np.uint32), np.zeros((H, W), np.int64)
    exp = contrib_ref._libm_exp
    with np.errstate(all="ignore"):
        for ty in range(r0_, r1_):
            for tx in range(gx):
                r0, r1 = (int(v) for v in ranges[ty * gx + tx])
                px, py, inside = FR._pixels(tx, ty, W, H)
                fx, fy = px.astype(F), py.astype(F)
                done = ~inside
                T = np.ones(256, F)
                D, M1, M2, m0 = (np.zeros(256, F) for _ in range(4))
                contrib, last, count = np.zeros(256, np.uint32), np.zeros(256, np.uint32), np.zeros(256, np.int64)
                for k in range(r0, max(r0, r1)):
                    if done.all():
                        break
                    g = int(lists[k])
                    act = ~done
                    contrib[act] += 1
                    gxy, con = means2D[g], co[g]
                    dx, dy = gxy[0] - fx, gxy[1] - fy
                    pw = F(-0.5) * (con[0] * dx * dx + con[2] * dy * dy) - con[1] * dx * dy
                    alpha = np.minimum(F(0.99), con[3] * exp(pw))
                    test = T * (F(1.0) - alpha)
                    live = act & ~(pw > 0) & ~(alpha < F(1.0) / F(255.0))
                    stop = live & (test < F(t_cutoff))
                    upd = live & ~stop
                    done |= stop
                    if upd.any():
                        m = val[g]
                        m0 = np.where(upd & (T == F(1.0)), m, m0).astype(F)
                        d = (m - m0).astype(F)
                        w = (alpha * T).astype(F)
                        Ap = (F(1.0) - T).astype(F)
                        if power == 2:
                            dd = (d * d).astype(F)
                            e = fma32(dd, Ap, fma32((F(-2.0) * d).astype(F), M1, M2))
                            M2 = np.where(upd, fma32(dd, w, M2), M2).astype(F)
                        else:
                            e = fma32(d, Ap, -M1)
                        D = np.where(upd, fma32(w, e, D), D).astype(F)
                        M1 = np.where(upd, fma32(d, w, M1), M1).astype(F)
                    T[upd] = test[upd]
                    last[upd] = contrib[upd]
                    count[upd] += 1
                ys, xs = py[inside], px[inside]
                out[ys, xs] = (F(2.0) * D)[inside]
                for plane, v in enumerate((m0, M1, M2)):
                    mom[plane, ys, xs] = v[inside]
                finalT[ys, xs] = T[inside]
                ncontrib[ys, xs] = last[inside]
                blended[ys, xs] = count[inside]
    return {"out": out, "moments": mom, "finalT": finalT, "nContrib": ncontrib, "blended": blended}


# ---- the float64 walk -----------------------------------------------------------------------------------------------------------
def _suffix(x):
    """sum over the records behind, exclusive: [L, P]."""
    return x.sum(axis=0)[None, :] - np.cumsum(x, axis=0)


def tile_walk(xy, co, vals, tx, ty, width, height, power, g_tile, moments_tile=None, t_cutoff=0.001, f32_forward=True,
              drop_suffix=False, f32_lines=False):
    """One 16 x 16 tile, [L records x 256 pixels]. vals [L]; g_tile [16,16]; moments_tile [3,16,16] (the float32 forward's m0,
    M1n, M2n, which the backward then takes as its inputs) or None: the walk's own, in float64.
    f32_forward=False: the forward in float64 too (the function finite differences are taken of).
    drop_suffix: dL/dalpha without its suffix term S inv — what a blind test would not see.
    f32_lines: the header's backward lines (d, dv, c, dL_dalpha, the suffix sums) in float32, operation by operation; the sums
    over the pixels stay in float64.
    Returns per record d_mean [L,2], d_conic [L,3], d_op [L,1], d_cov [L,3], d_val [L,1] and "M_" + each; n, pixels, free_pixels
    [L]; per pixel out, M_out [16,16] (float64 forward and its scale), final_t, n_contrib, blended."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    co = np.asarray(co, np.float64).reshape(-1, 4)
    vals = np.asarray(vals, np.float64).reshape(-1)
    L = xy.shape[0]
    ys, xs = np.mgrid[0:TILE, 0:TILE]
    px = (tx * TILE + xs).reshape(-1).astype(np.float64)
    py = (ty * TILE + ys).reshape(-1).astype(np.float64)
    inside = (px < width) & (py < height)
    gp = np.asarray(g_tile, np.float64).reshape(-1) * inside
    names = [name for name, _ in SUMS]
    if L == 0:
        res = {name: np.zeros((0, d)) for name, d in SUMS}
        res.update({"M_" + name: np.zeros((0, d)) for name, d in SUMS})
        zi = np.zeros(0, np.int64)
        z = np.zeros((TILE, TILE))
        res.update(n=zi, pixels=zi.copy(), free_pixels=zi.copy(), out=z, M_out=z.copy(), final_t=inside.astype(np.float64).reshape(TILE, TILE),
                   n_contrib=np.zeros((TILE, TILE), np.int64), blended=np.zeros((TILE, TILE), np.int64))
        return res
    from oracle import cpu_oracle
    f = np.float32
    dx = xy[:, 0:1] - px[None, :]
    dy = xy[:, 1:2] - py[None, :]
    A_, B_, C_, op = co[:, 0:1], co[:, 1:2], co[:, 2:3], co[:, 3:4]
    # the forward's decisions, in float32 in its operation order (features_ref.tile_backward)
    dx32, dy32 = f(xy[:, 0:1]) - f(px[None, :]), f(xy[:, 1:2]) - f(py[None, :])
    A32, B32, C32, op32 = f(A_), f(B_), f(C_), f(op)
    power_ = f(-0.5) * ((A32 * dx32) * dx32 + (C32 * dy32) * dy32) - (B32 * dx32) * dy32
    G = cpu_oracle.expf(np.minimum(power_, f(0.0))).reshape(power_.shape)
    raw = op32 * G
    alpha = np.minimum(f(0.99), raw)
    valid = (power_ <= 0.0) & (alpha >= f(1.0 / 255.0)) & inside[None, :]
    a_eff = np.where(valid, alpha, f(0.0))
    t_after = np.cumprod(f(1.0) - a_eff, axis=0, dtype=np.float32).astype(np.float64)
    power_, G, raw, alpha = (v.astype(np.float64) for v in (power_, G, raw, alpha))
    if not f32_forward:
        power_ = -0.5 * (A_ * dx * dx + C_ * dy * dy) - B_ * dx * dy
        G = np.exp(np.minimum(power_, 0.0))
        raw = op * G
        alpha = np.minimum(0.99, raw)
        valid = (power_ <= 0.0) & (alpha >= 1.0 / 255.0) & inside[None, :]
        t_after = np.cumprod(1.0 - np.where(valid, alpha, 0.0), axis=0)
    P = px.size
    t_before = np.vstack([np.ones((1, P)), t_after[:-1]])
    stop = valid & (t_after < t_cutoff)
    has_stop = stop.any(axis=0)
    stop_idx = np.where(has_stop, stop.argmax(axis=0), L)
    k = np.arange(L)[:, None]
    contrib = valid & (k < stop_idx[None, :])
    final_t = np.where(has_stop, t_before[np.minimum(stop_idx, L - 1), np.arange(P)], t_after[-1])
    w = np.where(contrib, alpha * t_before, 0.0)
    n_contrib = np.where(contrib.any(axis=0), L - np.argmax(contrib[::-1], axis=0), 0)
    blended = contrib.sum(axis=0)
    any_ = blended > 0
    first = np.argmax(contrib, axis=0)
    # the values centred on the pixel's first blended record; the moments: the kernel's inputs, or the walk's own
    if moments_tile is None:
        m0 = np.where(any_, vals[first], 0.0)
    else:
        mt = np.asarray(moments_tile, np.float64).reshape(3, -1)
        m0 = np.where(inside, mt[0], 0.0)
    d = np.where(contrib, vals[:, None] - m0[None, :], 0.0)
    ad = np.abs(d)
    if moments_tile is None:
        M1n, M2n = (w * d).sum(axis=0), (w * d * d).sum(axis=0)
    else:
        M1n, M2n = np.where(inside, mt[1], 0.0), np.where(inside, mt[2], 0.0)
    Ap, Ap_a = 1.0 - t_before, 1.0 + t_before
    # forward: e_i = sum_{j<i} w_j (d_i - d_j)^q from the prefix moments
    wd, wdd = w * d, w * d * d
    M1p_f, M2p_f = np.cumsum(wd, axis=0) - wd, np.cumsum(wdd, axis=0) - wdd
    M1p_fa = np.cumsum(w * ad, axis=0) - w * ad
    if power == 2:
        e = d * d * Ap - 2.0 * d * M1p_f + M2p_f
        e_a = d * d * Ap_a + 2.0 * ad * M1p_fa + M2p_f
    else:
        e = d * Ap - M1p_f
        e_a = ad * Ap_a + M1p_fa
    out = 2.0 * (w * e).sum(axis=0)
    M_out = 2.0 * (w * e_a).sum(axis=0)
    # backward
    one_minus = 1.0 - np.where(contrib, alpha, 0.0)
    aM1 = np.abs(M1n)
    if f32_lines:
        c, dm, dL_dalpha = _lines32(power, vals, m0, M1n, M2n, final_t, t_before, t_after, alpha, contrib, gp)
    else:
        if power == 2:
            An = 1.0 - final_t
            c = 2.0 * (d * d * An[None, :] - 2.0 * d * M1n[None, :] + M2n[None, :])
            dm = 4.0 * w * (d * An[None, :] - M1n[None, :])
        else:
            As = t_after - final_t[None, :]
            Ms = _suffix(wd)
            M1p = M1n[None, :] - Ms - wd
            c = 2.0 * ((d * Ap - M1p) + Ms - d * As)
            dm = 2.0 * w * (Ap - As)
        c = np.where(contrib, c, 0.0)
        S = _suffix(w * c)
        dL_dalpha = np.where(contrib, gp[None, :] * (t_before * c - (0.0 if drop_suffix else 1.0) * S / one_minus), 0.0)
    if power == 2:
        An_a = 1.0 + final_t
        c_a = 2.0 * (d * d * An_a[None, :] + 2.0 * ad * aM1[None, :] + np.abs(M2n)[None, :])
        dm_a = 4.0 * w * (ad * An_a[None, :] + aM1[None, :])
    else:
        As_a = t_after + final_t[None, :]
        Ms_a = _suffix(w * ad)
        M1p_a = aM1[None, :] + Ms_a + w * ad
        c_a = 2.0 * (ad * Ap_a + M1p_a + Ms_a + ad * As_a)
        dm_a = 2.0 * w * (Ap_a + As_a)
    c_a = np.where(contrib, c_a, 0.0)
    S_a = _suffix(w * c_a)
    free = contrib & ~(raw > 0.99)
    dLa = np.where(free, dL_dalpha, 0.0)
    dLa_a = np.where(free, np.abs(gp)[None, :] * (t_before * c_a + S_a / (1.0 - np.where(free, alpha, 0.0))), 0.0)
    dLp, dLp_a = op * G * dLa, op * G * dLa_a
    ux, uy = A_ * dx + B_ * dy, B_ * dx + C_ * dy
    adx, ady = np.abs(dx), np.abs(dy)
    uxa, uya = np.abs(A_) * adx + np.abs(B_) * ady, np.abs(B_) * adx + np.abs(C_) * ady
    res = {"d_val": (np.where(contrib, dm, 0.0) * gp[None, :]).sum(axis=1)[:, None],
           "d_op": (G * dLa).sum(axis=1)[:, None],
           "d_conic": np.stack([(-0.5 * dx * dx * dLp).sum(1), (-dx * dy * dLp).sum(1), (-0.5 * dy * dy * dLp).sum(1)], 1),
           "d_mean": np.stack([(-ux * dLp).sum(1), (-uy * dLp).sum(1)], 1),
           "d_cov": np.stack([(0.5 * ux * ux * dLp).sum(1), (0.5 * ux * uy * dLp).sum(1), (0.5 * uy * uy * dLp).sum(1)], 1),
           "M_d_val": (np.where(contrib, dm_a, 0.0) * np.abs(gp)[None, :]).sum(axis=1)[:, None],
           "M_d_op": (G * dLa_a).sum(axis=1)[:, None],
           "M_d_conic": np.stack([(0.5 * adx * adx * dLp_a).sum(1), (adx * ady * dLp_a).sum(1), (0.5 * ady * ady * dLp_a).sum(1)], 1),
           "M_d_mean": np.stack([(uxa * dLp_a).sum(1), (uya * dLp_a).sum(1)], 1),
           "M_d_cov": np.stack([(0.5 * uxa * uxa * dLp_a).sum(1), (0.5 * uxa * uya * dLp_a).sum(1), (0.5 * uya * uya * dLp_a).sum(1)], 1)}
    assert set(names) == {k_ for k_ in res if not k_.startswith("M_")}
    res.update(n=np.where(contrib, blended[None, :], 0).max(axis=1), pixels=contrib.sum(axis=1), free_pixels=free.sum(axis=1),
               out=np.where(inside, out, 0.0).reshape(TILE, TILE), M_out=np.where(inside, M_out, 0.0).reshape(TILE, TILE),
               final_t=np.where(inside, final_t, 0.0).reshape(TILE, TILE), n_contrib=n_contrib.reshape(TILE, TILE),
               blended=blended.reshape(TILE, TILE), w=w, contrib=contrib)
    return res


def _lines32(power, vals, m0, M1n, M2n, final_t, t_before, t_after, alpha, contrib, gp):
    """The header's backward lines in float32, record by record from the back: (c, dm, dL_dalpha) [L,P] as float64 arrays of
    float32 values. Tn and w are the forward's (t_before, alpha t_before) rounded to float32; inv = 1 / (1 - alpha) in float32."""
    L, P = contrib.shape
    f = F
    m0, M1n, M2n, Tf, g = f(m0), f(M1n), f(M2n), f(final_t), f(gp)
    An = (f(1.0) - Tf).astype(f)
    S, Ms, Tb = np.zeros(P, f), np.zeros(P, f), Tf.copy()
    c_o, dm_o, da_o = np.zeros((L, P)), np.zeros((L, P)), np.zeros((L, P))
    with np.errstate(all="ignore"):
        for i in range(L - 1, -1, -1):
            act = contrib[i]
            if not act.any():
                continue
            a = f(alpha[i])
            inv = (f(1.0) / (f(1.0) - a)).astype(f)
            Tn = f(t_before[i])
            w = np.where(act, (a * Tn).astype(f), f(0.0)).astype(f)
            d = (f(vals[i]) - m0).astype(f)
            if power == 2:
                t = fma32(d, An, -M1n)
                dv = (f(4.0) * t).astype(f)
                c = (f(2.0) * fma32((d * d).astype(f), An, fma32((f(-2.0) * d).astype(f), M1n, M2n))).astype(f)
            else:
                As, Ap = (Tb - Tf).astype(f), (f(1.0) - Tn).astype(f)
                dv = (f(2.0) * (Ap - As).astype(f)).astype(f)
                M1p = ((M1n - Ms).astype(f) - (w * d).astype(f)).astype(f)
                c = (f(2.0) * (((fma32(d, Ap, -M1p) + Ms).astype(f)) - (d * As).astype(f)).astype(f)).astype(f)
                Ms = np.where(act, fma32(w, d, Ms), Ms).astype(f)
                Tb = np.where(act, Tn, Tb).astype(f)
            da = (g * fma32(Tn, c, -((S * inv).astype(f)))).astype(f)
            S = np.where(act, fma32(c, w, S), S).astype(f)
            c_o[i] = np.where(act, c, 0.0)
            dm_o[i] = np.where(act, (w.astype(np.float64) * dv.astype(np.float64)), 0.0)
            da_o[i] = np.where(act, da, 0.0)
    return c_o, dm_o, da_o


def frame_walk(state, values, power, g, W, H, moments=None, t_cutoff=0.001, tile_rows=None, **kw):
    """tile_walk over the tiles of rows `tile_rows` (default: all) of a forward state, summed per Gaussian: d_* and M_d_* [N,.],
    n (the maximum over the tiles), pixels, free_pixels [N]; out, M_out, final_t [H,W] (NaN outside the rows), n_contrib (-1),
    blended [H,W]. g [H,W]; moments [3,H,W] (forward32's, or the GPU's) or None."""
    means2D = np.asarray(state["means2D"], np.float32).reshape(-1, 2)
    conic = np.asarray(state["conicOpacity"], np.float32).reshape(-1, 4)
    val = np.asarray(values)
    val = val.astype(np.float32) if val.dtype != np.float64 else val
    n = means2D.shape[0]
    g = np.asarray(g, np.float64).reshape(H, W)
    ranges = np.asarray(state["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    lists = np.asarray(state["values"]).view(np.uint32).astype(np.int64)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r0, r1 = (0, gy) if tile_rows is None else tile_rows
    names = [name for name, _ in SUMS]
    dims = dict(SUMS)
    out = {name: np.zeros((n, dims[name])) for name in names}
    out.update({"M_" + name: np.zeros((n, dims[name])) for name in names})
    out.update(n=np.zeros(n, np.int64), pixels=np.zeros(n, np.int64), free_pixels=np.zeros(n, np.int64),
               out=np.full((H, W), np.nan), M_out=np.full((H, W), np.nan), final_t=np.full((H, W), np.nan),
               n_contrib=np.full((H, W), -1, np.int64), blended=np.zeros((H, W), np.int64))
    for ty in range(r0, r1):
        for tx in range(gx):
            a, b = (int(v) for v in ranges[ty * gx + tx])
            ids = lists[a:b] if b > a else lists[0:0]
            ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
            tile_g = np.zeros((16, 16))
            tile_g[: yb - ya, : xb - xa] = g[ya:yb, xa:xb]
            tile_m = None
            if moments is not None:
                tile_m = np.zeros((3, 16, 16))
                tile_m[:, : yb - ya, : xb - xa] = np.asarray(moments, np.float64)[:, ya:yb, xa:xb]
            res = tile_walk(means2D[ids], conic[ids], val[ids], tx, ty, W, H, power, tile_g, tile_m, t_cutoff, **kw)
            for name in names:
                np.add.at(out[name], ids, res[name])
                np.add.at(out["M_" + name], ids, res["M_" + name])
            for key in ("pixels", "free_pixels"):
                np.add.at(out[key], ids, res[key])
            np.maximum.at(out["n"], ids, res["n"])
            for key in ("out", "M_out", "final_t", "n_contrib", "blended"):
                out[key][ya:yb, xa:xb] = res[key][: yb - ya, : xb - xa]
    return out


def bound(ref, name):
    """BW_TAU (n + BW_C) M + BW_ATOL per Gaussian and component: helpers.py's rule and constants, n in place of k."""
    from helpers import BW_ATOL, BW_C, BW_TAU
    return BW_TAU * (ref["n"].astype(np.float64) + BW_C)[:, None] * ref["M_" + name] + BW_ATOL


def worst_ratio(got, ref, name):
    """max |got - ref| / ((n + BW_C) M) over the components with M > 0."""
    from helpers import BW_C
    got = np.asarray(got, np.float64).reshape(ref[name].shape)
    err = np.abs(got - ref[name])
    scale = (ref["n"].astype(np.float64) + BW_C)[:, None] * ref["M_" + name]
    ratio = np.where(ref["M_" + name] > 0, err / np.maximum(scale, 1e-300), 0.0)
    return float(ratio.max()) if ratio.size else 0.0

