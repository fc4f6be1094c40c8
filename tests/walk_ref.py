"""The two walks over a tile's sorted list that the references of the list-walk passes share, each written once, as
gsrast_amd/csrc/list_walk.hpp holds them once for the kernels: contrib_ref, median_ref, features_ref and distortion_ref (forward)
take the replay; absgrad_ref, features_ref and distortion_ref (backward) the back walk, with geometry_sums behind it. A pass's
own lines stay in its own file and come in as callables.

What is RESTATED here, and must agree with it:
  - replay (front to back, float32): blend_core.hpp's composite_record — the reference-order power, alpha = min(0.99, o e),
    `power > 0`, `alpha < 1/255`, T = T (1 - alpha) and the cut-off test — with the masks and the operation order of
    oracle/oracle_np.py's blend loop and exp = the C++ oracle's libm expf.
  - tile_decisions, geometry_sums (back to front, float64 over the float32 decisions, [L records x 256 pixels]):
    render_backward_kernel (backward.hip) and list_walk.hpp's GeometrySums, as oracle/backward_np.blend_tile_backward states
    them for three colour channels with f32_forward=True, magnitudes=True: the decisions, `free` (raw > 0.99 zeroes a pixel's
    share of the geometry but not the walk), u = K d, the sums, their condition scales M (every factor replaced by its
    absolute value) and the walk depth k.
oracle/backward_np.blend_tile_backward and cpu_oracle.forward are kept APART on purpose: this file imports neither for its
arithmetic, and tests/test_walk_ref_cpu.py pins it against both, so that the references built on it stand on an independent anchor."""
import types

import numpy as np

F = np.float32
TILE = 16
T_CUTOFF = {"gscuda": 0.001, "inria": 0.0001}
GEOMETRY = (("d_mean", 2), ("d_conic", 3), ("d_op", 1), ("d_cov", 3))      # the geometry sums, in the order of sums_f64's slots 0..5, 9..11


def libm_exp(x):
    from oracle import cpu_oracle
    return cpu_oracle.expf(x)


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


def ulp32(x):
    """The spacing of float32 at |x| (float64 in, float64 out; the smallest normal's for anything below it)."""
    a = np.maximum(np.abs(np.asarray(x, np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)).astype(np.float64) - a.astype(np.float64))


def depth_values(means3D, view, inverse=False):
    """d_i as the blend computes it (blend_core.hpp: depth_value), float32 in its operation order."""
    m, v = np.asarray(means3D, F), np.asarray(view, F).reshape(-1)
    z = (v[2] * m[:, 0] + v[6] * m[:, 1]) + (v[10] * m[:, 2] + v[14] * F(1.0))
    with np.errstate(all="ignore"):
        return (F(1.0) / z).astype(F) if inverse else z.astype(F)


def _pixels(tx, ty, W, H):
    ly, lx = np.divmod(np.arange(256), 16)
    px, py = tx * 16 + lx, ty * 16 + ly
    return px, py, (px < W) & (py < H)


def _lists(ranges, lists):
    return (np.asarray(ranges).view(np.uint32).reshape(-1, 2).astype(np.int64), np.asarray(lists).view(np.uint32).astype(np.int64))


def _band(tile_rows, H):
    return (0, (H + 15) // 16) if tile_rows is None else tile_rows


def with_scales(sums):
    """(name, width) of a pass's sums and of the condition scale "M_" + name of each."""
    return tuple(sums) + tuple(("M_" + name, d) for name, d in sums)


# ---- the replay, front to back, float32 -----------------------------------------------------------------------------------------
def replay(means2D, conic_opacity, ranges, lists, W, H, t_cutoff=0.001, tile_rows=None, exp=None,
           start=lambda tx, ty: None, record=lambda *a: None, end=lambda *a: None):
    """finalT [H,W] float32, nContrib [H,W] uint32, stopped [H,W] bool (the pixel ended on the cut-off) of the blend loop over the
    tiles of rows `tile_rows` (default: all; zeros outside). The pass's part:
    start(tx, ty) -> the pass's per-tile registers `regs` (anything);
    record(regs, g, pos, con, dx, dy, power, alpha, T, upd) for every record that some pixel BLENDS: the Gaussian g, its 1-based
        position in the tile's list, its conic and opacity, dx, dy, power, alpha [256] float32, T the transmittance in front of
        the record and upd the mask of the pixels that blend it (all [256]; only `regs` may be written);
    end(regs, px, py, inside, T, last, done) once the list is walked, to scatter: T the final transmittance, last the position
        of the pixel's last blended record, done whether it stopped."""
    exp = libm_exp if exp is None else exp
    means2D = np.asarray(means2D, F).reshape(-1, 2)
    co = np.asarray(conic_opacity, F).reshape(-1, 4)
    ranges, lists = _lists(ranges, lists)
    gx = (W + 15) // 16
    finalT, ncontrib, stopped = np.zeros((H, W), F), np.zeros((H, W), np.uint32), np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for ty in range(*_band(tile_rows, H)):
            for tx in range(gx):
                r0, r1 = (int(v) for v in ranges[ty * gx + tx])
                px, py, inside = _pixels(tx, ty, W, H)
                fx, fy = px.astype(F), py.astype(F)
                done = ~inside
                T = np.ones(256, F)
                contrib, last = np.zeros(256, np.uint32), np.zeros(256, np.uint32)
                regs = start(tx, ty)
                for k in range(r0, max(r0, r1)):
                    if done.all():
                        break
                    g = int(lists[k])
                    act = ~done
                    contrib[act] += 1
                    gxy, con = means2D[g], co[g]
                    dx, dy = gxy[0] - fx, gxy[1] - fy
                    power = F(-0.5) * (con[0] * dx * dx + con[2] * dy * dy) - con[1] * dx * dy
                    alpha = np.minimum(F(0.99), con[3] * exp(power))
                    test = T * (F(1.0) - alpha)
                    live = act & ~(power > 0) & ~(alpha < F(1.0) / F(255.0))
                    stop = live & (test < F(t_cutoff))
                    upd = live & ~stop                                   # the record is BLENDED into these pixels
                    done |= stop
                    if upd.any():
                        record(regs, g, k - r0 + 1, con, dx, dy, power, alpha, T, upd)
                    T[upd] = test[upd]
                    last[upd] = contrib[upd]
                ys, xs = py[inside], px[inside]
                finalT[ys, xs] = T[inside]
                ncontrib[ys, xs] = last[inside]
                stopped[ys, xs] = done[inside]
                end(regs, px, py, inside, T, last, done)
    return finalT, ncontrib, stopped


# ---- the back walk, float64 over the float32 decisions --------------------------------------------------------------------------
def tile_decisions(xy, co, tx, ty, width, height, t_cutoff=0.001, f32_forward=True):
    """One 16 x 16 tile, [L records x 256 pixels]: what the forward decided, as float64 arrays of the float32 forward's values
    (blend_tile_backward's f32_forward semantics: power, exp = libm's expf, alpha and the transmittance product in float32 in
    the forward's operation order, GSCuda.cu:634-657; f32_forward=False: the forward in float64 too, the function finite
    differences can be taken of). Returns a namespace: L, px, py, inside [256]; for L > 0 also dx, dy [L,256], A_, B_, C_, op
    [L,1], G, raw, alpha, contrib, free (blended, and blended with raw <= 0.99), t_before, t_after, w [L,256], final_t,
    n_contrib, blended [256], and per record the walk depth k, pixels, free_pixels [L]."""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    co = np.asarray(co, np.float64).reshape(-1, 4)
    L = xy.shape[0]
    px, py, inside = _pixels(tx, ty, width, height)
    px, py = px.astype(np.float64), py.astype(np.float64)
    d = types.SimpleNamespace(L=L, px=px, py=py, inside=inside)
    if L == 0:
        return d
    f = np.float32
    dx = xy[:, 0:1] - px[None, :]
    dy = xy[:, 1:2] - py[None, :]
    A_, B_, C_, op = co[:, 0:1], co[:, 1:2], co[:, 2:3], co[:, 3:4]
    if f32_forward:
        dx32, dy32 = f(xy[:, 0:1]) - f(px[None, :]), f(xy[:, 1:2]) - f(py[None, :])
        A32, B32, C32, op32 = f(A_), f(B_), f(C_), f(op)
        power = f(-0.5) * ((A32 * dx32) * dx32 + (C32 * dy32) * dy32) - (B32 * dx32) * dy32
        G = libm_exp(np.minimum(power, f(0.0))).reshape(power.shape)
        raw = op32 * G
        alpha = np.minimum(f(0.99), raw)
        valid = (power <= 0.0) & (alpha >= f(1.0 / 255.0)) & inside[None, :]
        a_eff = np.where(valid, alpha, f(0.0))
        t_after = np.cumprod(f(1.0) - a_eff, axis=0, dtype=np.float32).astype(np.float64)
        G, raw, alpha = (v.astype(np.float64) for v in (G, raw, alpha))
    else:
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
    contrib = valid & (np.arange(L)[:, None] < stop_idx[None, :])
    free = contrib & ~(raw > 0.99)
    walk = np.cumsum(contrib[::-1], axis=0)[::-1]
    d.__dict__.update(
        dx=dx, dy=dy, A_=A_, B_=B_, C_=C_, op=op, G=G, raw=raw, alpha=alpha, contrib=contrib, free=free, t_before=t_before,
        t_after=t_after, final_t=np.where(has_stop, t_before[np.minimum(stop_idx, L - 1), np.arange(px.size)], t_after[-1]),
        w=np.where(contrib, alpha * t_before, 0.0), n_contrib=np.where(contrib.any(axis=0), L - np.argmax(contrib[::-1], axis=0), 0),
        k=np.where(contrib, walk, 0).max(axis=1), pixels=contrib.sum(axis=1), free_pixels=free.sum(axis=1), blended=contrib.sum(axis=0))
    return d


def geometry_sums(d, dL_dalpha, dLa_a, shares=False):
    """d_mean [L,2], d_conic [L,3], d_op [L,1], d_cov [L,3] and "M_" + each of a pass's dL_dalpha [L,256] (taken on the free
    pixels) and of its absolute counterpart dLa_a (zero off them already). shares: also A_d_mean [L,2], the sum over the
    pixels of |the pixel's share of d_mean|."""
    dLa = np.where(d.free, dL_dalpha, 0.0)
    dx, dy, G = d.dx, d.dy, d.G
    dLp, dLp_a = d.op * G * dLa, d.op * G * dLa_a
    ux, uy = d.A_ * dx + d.B_ * dy, d.B_ * dx + d.C_ * dy
    sx, sy = -ux * dLp, -uy * dLp                                        # the pixel's share of dL/d mean2D
    adx, ady = np.abs(dx), np.abs(dy)
    uxa, uya = np.abs(d.A_) * adx + np.abs(d.B_) * ady, np.abs(d.B_) * adx + np.abs(d.C_) * ady
    res = {"d_op": (G * dLa).sum(axis=1)[:, None],
           "d_conic": np.stack([(-0.5 * dx * dx * dLp).sum(1), (-dx * dy * dLp).sum(1), (-0.5 * dy * dy * dLp).sum(1)], 1),
           "d_mean": np.stack([sx.sum(1), sy.sum(1)], 1),
           "d_cov": np.stack([(0.5 * ux * ux * dLp).sum(1), (0.5 * ux * uy * dLp).sum(1), (0.5 * uy * uy * dLp).sum(1)], 1),
           "M_d_op": (G * dLa_a).sum(axis=1)[:, None],
           "M_d_conic": np.stack([(0.5 * adx * adx * dLp_a).sum(1), (adx * ady * dLp_a).sum(1), (0.5 * ady * ady * dLp_a).sum(1)], 1),
           "M_d_mean": np.stack([(uxa * dLp_a).sum(1), (uya * dLp_a).sum(1)], 1),
           "M_d_cov": np.stack([(0.5 * uxa * uxa * dLp_a).sum(1), (0.5 * uxa * uya * dLp_a).sum(1), (0.5 * uya * uya * dLp_a).sum(1)], 1)}
    if shares:
        res["A_d_mean"] = np.stack([np.abs(sx).sum(1), np.abs(sy).sum(1)], 1)
    return res


def tile_maps(d):
    """pixels, free_pixels [L] and final_t, n_contrib [16,16] (0 outside the image) of the decisions, an empty list's included."""
    if d.L == 0:
        zi = np.zeros(0, np.int64)
        return dict(pixels=zi, free_pixels=zi.copy(), final_t=d.inside.astype(np.float64).reshape(TILE, TILE),
                    n_contrib=np.zeros((TILE, TILE), np.int64))
    return dict(pixels=d.pixels, free_pixels=d.free_pixels, final_t=np.where(d.inside, d.final_t, 0.0).reshape(TILE, TILE),
                n_contrib=d.n_contrib.reshape(TILE, TILE))


def empty_tile(d, sums, depth, **maps):
    """What a tile whose list is empty returns: zeros [0, width] of every (name, width) of `sums`, no depths, tile_maps and the
    pass's own per-pixel `maps`."""
    res = {name: np.zeros((0, width)) for name, width in sums}
    res[depth] = np.zeros(0, np.int64)
    res.update(tile_maps(d), **maps)
    return res


def frame(state, W, H, tile_rows, pixel_inputs, tile, sums, depth, maps=(), tiles=False, prefix=False):
    """A pass's tile function over the tiles of rows `tile_rows` (default: all) of a forward state (means2D, conicOpacity, ranges,
    values: cpu_oracle.forward's dict or the GPU's arrays under those names), summed per Gaussian.
    pixel_inputs: {name: float64 [..., H, W] or None}; tile(xy, co, ids, tx, ty, **padded) gets the records of the tile's list
    and each input's 16 x 16 tile, zero past the image's edge (None stays None).
    Returns the float64 sums [N, width] of `sums`, pixels / free_pixels [N] and `depth` [N] (the maximum over the tiles) int64,
    tiles [N] where asked (the tiles in which some pixel blended the Gaussian), final_t [H,W] (NaN outside the rows), n_contrib
    [H,W] (-1 there) and every (name, fill) of `maps` [H,W]: float64 for a NaN fill, int64 for another.
    prefix: walk each tile's list only as far as state["nContrib"] reaches."""
    means2D = np.asarray(state["means2D"], np.float32).reshape(-1, 2)
    conic = np.asarray(state["conicOpacity"], np.float32).reshape(-1, 4)
    ranges, lists = _lists(state["ranges"], state["values"])
    n = means2D.shape[0]
    gx = (W + 15) // 16
    counts = ("pixels", "free_pixels")
    out = {name: np.zeros((n, width)) for name, width in sums}
    out.update({name: np.zeros(n, np.int64) for name in counts + (depth,) + (("tiles",) if tiles else ())})
    maps = (("final_t", np.nan), ("n_contrib", -1)) + tuple(maps)
    out.update({name: np.full((H, W), fill, np.float64 if fill != fill else np.int64) for name, fill in maps})
    for ty in range(*_band(tile_rows, H)):
        for tx in range(gx):
            a, b = (int(v) for v in ranges[ty * gx + tx])
            ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
            if prefix and b > a:
                b = min(b, a + int(np.asarray(state["nContrib"]).view(np.uint32).reshape(H, W)[ya:yb, xa:xb].max()))
            ids = lists[a:b] if b > a else lists[0:0]
            padded = dict.fromkeys(pixel_inputs)
            for name, v in pixel_inputs.items():
                if v is not None:
                    padded[name] = np.zeros(v.shape[:-2] + (16, 16))
                    padded[name][..., : yb - ya, : xb - xa] = v[..., ya:yb, xa:xb]
            res = tile(means2D[ids], conic[ids], ids, tx, ty, **padded)
            for name in tuple(name for name, _ in sums) + counts:
                np.add.at(out[name], ids, res[name])
            np.maximum.at(out[depth], ids, res[depth])
            if tiles:
                np.add.at(out["tiles"], ids, (res["pixels"] > 0).astype(np.int64))
            for name, _ in maps:
                out[name][ya:yb, xa:xb] = res[name][: yb - ya, : xb - xa]
    return out
