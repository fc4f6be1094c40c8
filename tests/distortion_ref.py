"""Reference of the depth distortion map (include/gsrast_amd_distortion.h), shared by tests/test_distortion_cpu.py and
tests/test_gpu_distortion.py with the scenes (absgrad_ref.all_scenes, imported), the values and the pixel gradients both use.

forward32: the float32 restatement of the header's forward, line for line, as hooks of walk_ref.replay (the masks, the
power, exp = libm's expf, alpha, the cut-off) with every fmaf rounded once (walk_ref.fma32). The GPU's out and moments are
compared with it bit for bit.
tile_walk: a float64 walk, forward and backward, over the float32 forward's decisions (walk_ref.tile_decisions': power,
exp, alpha and the transmittance product in float32), handed the float32 moments m0, M1n, M2n the kernel reads — the header's
formulas in exact arithmetic on the kernel's own inputs. Per record it returns every sum, its condition scale M — the same sum
with every factor and every subtraction taken in absolute value: 1 - T counts as 1 + T, T_{i+1} - T_f as their sum, c as the sum
of its summands' magnitudes — and n, the largest number of records blended into any pixel that blended the record.
Acceptance is helpers.py's rule with n in place of k (each term uses totals over the pixel's whole list, not over the records
behind it):  |got - exp| <= BW_TAU (n + BW_C) M + BW_ATOL."""
import types

import numpy as np

import absgrad_ref as A
import features_ref as FR
import walk_ref
from walk_ref import T_CUTOFF, TILE, fma32      # noqa: F401  (T_CUTOFF: a name the callers take from here)

F = np.float32
POWERS = (2, 1)
SUMS = FR.SUMS + (("d_val", 1),)
MAPS = (("out", np.nan), ("M_out", np.nan), ("blended", 0))      # the walk's per-pixel maps beside final_t / n_contrib, and their fill


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
    val = np.asarray(values, F).reshape(-1)
    out, mom, blended = np.full((H, W), np.nan, F), np.full((3, H, W), np.nan, F), np.zeros((H, W), np.int64)

    def start(tx, ty):
        D, M1, M2, m0 = (np.zeros(256, F) for _ in range(4))
        return types.SimpleNamespace(D=D, M1=M1, M2=M2, m0=m0, count=np.zeros(256, np.int64))

    def record(r, g, pos, con, dx, dy, pw, alpha, T, upd):
        m = val[g]
        r.m0 = np.where(upd & (T == F(1.0)), m, r.m0).astype(F)
        d = (m - r.m0).astype(F)
        w = (alpha * T).astype(F)
        Ap = (F(1.0) - T).astype(F)
        if power == 2:
            dd = (d * d).astype(F)
            e = fma32(dd, Ap, fma32((F(-2.0) * d).astype(F), r.M1, r.M2))
            r.M2 = np.where(upd, fma32(dd, w, r.M2), r.M2).astype(F)
        else:
            e = fma32(d, Ap, -r.M1)
        r.D = np.where(upd, fma32(w, e, r.D), r.D).astype(F)
        r.M1 = np.where(upd, fma32(d, w, r.M1), r.M1).astype(F)
        r.count[upd] += 1

    def end(r, px, py, inside, T, last, done):
        ys, xs = py[inside], px[inside]
        out[ys, xs] = (F(2.0) * r.D)[inside]
        for plane, v in enumerate((r.m0, r.M1, r.M2)):
            mom[plane, ys, xs] = v[inside]
        blended[ys, xs] = r.count[inside]

    finalT, ncontrib, _ = walk_ref.replay(state["means2D"], state["conicOpacity"], state["ranges"], state["values"], W, H, t_cutoff,
                                          tile_rows, None, start, record, end)
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
    dec = walk_ref.tile_decisions(xy, co, tx, ty, width, height, t_cutoff, f32_forward)
    if dec.L == 0:
        z = np.zeros((TILE, TILE))
        return walk_ref.empty_tile(dec, walk_ref.with_scales(SUMS), "n", out=z, M_out=z.copy(), blended=np.zeros((TILE, TILE), np.int64))
    vals = np.asarray(vals, np.float64).reshape(-1)
    inside, contrib, free, alpha, w, blended = dec.inside, dec.contrib, dec.free, dec.alpha, dec.w, dec.blended
    t_before, t_after, final_t = dec.t_before, dec.t_after, dec.final_t
    gp = np.asarray(g_tile, np.float64).reshape(-1) * inside
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
    dLa_a = np.where(free, np.abs(gp)[None, :] * (t_before * c_a + S_a / (1.0 - np.where(free, alpha, 0.0))), 0.0)
    res = walk_ref.geometry_sums(dec, dL_dalpha, dLa_a)
    res.update(walk_ref.tile_maps(dec), d_val=(np.where(contrib, dm, 0.0) * gp[None, :]).sum(axis=1)[:, None],
               M_d_val=(np.where(contrib, dm_a, 0.0) * np.abs(gp)[None, :]).sum(axis=1)[:, None],
               n=np.where(contrib, blended[None, :], 0).max(axis=1), out=np.where(inside, out, 0.0).reshape(TILE, TILE),
               M_out=np.where(inside, M_out, 0.0).reshape(TILE, TILE), blended=blended.reshape(TILE, TILE), w=w, contrib=contrib)
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
    val = np.asarray(values)
    val = val.astype(np.float32) if val.dtype != np.float64 else val

    def tile(xy, co, ids, tx, ty, g, moments):
        return tile_walk(xy, co, val[ids], tx, ty, W, H, power, g, moments, t_cutoff, **kw)

    return walk_ref.frame(state, W, H, tile_rows, {"g": np.asarray(g, np.float64).reshape(H, W),
                                                   "moments": None if moments is None else np.asarray(moments, np.float64)},
                          tile, walk_ref.with_scales(SUMS), "n", MAPS)


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

