"""CPU: the N-channel feature maps (gsr_features_forward / gsr_features_backward, include/gsrast_amd_features.h). The reference
of tests/features_ref.py by hand on a two-record tile; its forward replay against the project's oracle (colour and finalT bit for
bit with features = colours); its gradients against finite differences of the float64 forward, for the features and for every
geometry sum; the superposition identity against oracle/backward_np.blend_tile_backward and tests/absgrad_ref's `signed`; the
blindness guards of the scenes tests/test_gpu_features.py uses; the ninth header against its ctypes table; every refusal of the
two calls without a device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import absgrad_ref as A
import features_ref as R
from helpers import ROOT
from oracle import backward_np as B
from oracle import cpu_oracle

from gsrast_amd import _capi

SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}


@functools.lru_cache(maxsize=None)
def state_of(name):
    scene, cam = SCENES[name]
    return cpu_oracle.forward(scene, cam, background=R.BACKGROUND)


def _close(a, b, what, rel=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert (np.abs(a - b) <= rel * np.maximum(np.abs(a), np.abs(b)) + 1e-300).all(), (what, float(np.abs(a - b).max()))


# ---- 1. by hand ---------------------------------------------------------------------------------------------------------------
def test_two_records_on_one_pixel_by_hand():
    """Two records over pixel (0, 0) of a 1 x 1 image, C = 2, written out: w1 = a1, w2 = a2 (1 - a1), T_f = (1 - a1)(1 - a2)."""
    f = np.float32
    xy = np.array([[0.5, 0.25], [0.25, -0.5]], f)
    co = np.array([[0.5, 0.125, 0.75, 0.5], [0.25, 0.0, 0.5, 0.75]], f)
    feat = np.array([[0.25, -1.0], [2.0, 0.5]], f)
    bg, g = np.array([0.5, -0.25]), np.array([1.0, -2.0])
    gt = np.zeros((2, 16, 16))
    gt[:, 0, 0] = g
    res = R.tile_backward(xy, co, feat, 0, 0, 1, 1, bg, gt)
    a, G = [], []
    for (x, y), (A_, B_, C_, o) in zip(xy, co):
        power = f(-0.5) * ((A_ * x) * x + (C_ * y) * y) - (B_ * x) * y
        G.append(float(cpu_oracle.expf(np.array([power], f))[0]))
        a.append(float(f(o) * f(G[-1])))
    t1 = float(f(1) - f(a[0]))
    tf = float(f(t1) * (f(1) - f(a[1])))
    w = [a[0], a[1] * t1]
    feat32, feat = feat, feat.astype(np.float64)
    assert res["n_contrib"][0, 0] == 2 and res["final_t"][0, 0] == tf and list(res["pixels"]) == [1, 1] and list(res["k"]) == [2, 1]
    _close(res["out"][:, 0, 0], w[0] * feat[0] + w[1] * feat[1] + tf * bg, "out")
    _close(res["d_chan"], np.outer(w, g), "d_chan")
    # dL/dalpha_2 = T_2 (f_2 . g) - T_f (bg . g) / (1 - a_2);  dL/dalpha_1 = (f_1 . g) - (w_2 (f_2 . g) + T_f (bg . g)) / (1 - a_1)
    d2 = t1 * float(feat[1] @ g) - tf * float(bg @ g) / (1 - a[1])
    d1 = float(feat[0] @ g) - (w[1] * float(feat[1] @ g) + tf * float(bg @ g)) / (1 - a[0])
    _close(res["d_op"][:, 0], [G[0] * d1, G[1] * d2], "d_op")
    for i, d in enumerate((d1, d2)):
        x, y = (float(v) for v in xy[i])
        A_, B_, C_, o = (float(v) for v in co[i])
        dp = o * G[i] * d                     # (d power: opacity x G in float64, not the float32 alpha)
        ux, uy = A_ * x + B_ * y, B_ * x + C_ * y
        _close(res["d_mean"][i], [-ux * dp, -uy * dp], "d_mean")
        _close(res["d_conic"][i], [-0.5 * x * x * dp, -x * y * dp, -0.5 * y * y * dp], "d_conic")
        _close(res["d_cov"][i], [0.5 * ux * ux * dp, 0.5 * ux * uy * dp, 0.5 * uy * uy * dp], "d_cov")
    # the float32 replay of the same tile
    state = {"means2D": xy, "conicOpacity": co, "ranges": np.array([[0, 2]], np.uint32), "values": np.array([0, 1], np.uint32)}
    fw = R.forward(state, feat32, bg.astype(f), 1, 1)
    acc = R.fma32(feat32[1], f(f(a[1]) * f(t1)), R.fma32(feat32[0], f(f(a[0]) * f(1)), np.zeros(2, f)))
    assert fw["nContrib"][0, 0] == 2 and fw["finalT"][0, 0] == f(tf)
    assert np.array_equal(fw["out"][:, 0, 0], (acc + (f(tf) * bg.astype(f)).astype(f)).astype(f))


def test_fma32_rounds_once():
    f = np.float32
    a, b = f(1.0 + 2.0 ** -12), f(1.0 + 2.0 ** -12)          # a b = 1 + 2^-11 + 2^-24: the last term is half an ulp of 1
    assert R.fma32(a, b, f(-1.0)) == f(2.0 ** -11 + 2.0 ** -24) and f(a * b) + f(-1.0) == f(2.0 ** -11)
    # a tie in float64 that is not one exactly: 1 + 2^-24 (a float32 midpoint) plus 2^-60 must round up
    assert R.fma32(f(2.0 ** -30), f(2.0 ** -30), np.float64(1.0 + 2.0 ** -24)) == f(1.0 + 2.0 ** -23)
    rng = np.random.default_rng(0)
    x, y, z = (rng.normal(size=4096).astype(f) for _ in range(3))
    import fractions
    for i in range(0, 4096, 64):
        exact = fractions.Fraction(float(x[i])) * fractions.Fraction(float(y[i])) + fractions.Fraction(float(z[i]))
        lo = R.fma32(x[i], y[i], z[i])
        near = [np.nextafter(lo, f(-np.inf)), lo, np.nextafter(lo, f(np.inf))]
        assert min(near, key=lambda v: abs(fractions.Fraction(float(v)) - exact)) == lo


# ---- 2. the forward replay is the oracle's blend --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_replay_with_the_colours_is_the_oracles_image_bit_for_bit(name):
    """The oracle's colour sums are the reference's, acc + (c * alpha) * T in three roundings; the blend kernels' — and so this
    pass's — are fmaf(c, alpha T, acc) in two (blend_core.hpp: they feed no test). The replay in the oracle's form is the oracle's
    image bit for bit, which pins its walk, alpha, T and decisions; the fused form shares all of that (finalT and nContrib bit for
    bit) and differs by the roundings alone: per blended record at most 3 x 2^-24 of a term and a running sum that are both
    below 1 (colours in [0.1, 0.9], weights that add up to at most 1), i.e. |difference| <= (nContrib + 1) 2^-22."""
    scene, cam = SCENES[name]
    st = state_of(name)
    bg = np.asarray(R.BACKGROUND, np.float32)
    exact = R.forward(st, st["rgb"], bg, cam.width, cam.height, fused=False)
    fw = R.forward(st, st["rgb"], bg, cam.width, cam.height)
    want = np.asarray(st["out_color"], np.float32)
    for got in (exact, fw):
        assert np.array_equal(got["finalT"].view(np.uint32), np.asarray(st["finalT"], np.float32).view(np.uint32)), "finalT"
        assert np.array_equal(got["nContrib"], np.asarray(st["nContrib"]).view(np.uint32)), "nContrib"
    assert np.array_equal(exact["out"].view(np.uint32), want.view(np.uint32)), "out_color"
    assert np.abs(st["rgb"]).max() < 1.0 and np.abs(bg).max() < 1.0
    assert (np.abs(fw["out"].astype(np.float64) - want) <= (fw["nContrib"][None] + 1.0) * 2.0 ** -22).all()


# ---- 3. gradients against finite differences of the float64 forward ------------------------------------------------------
def _fd_tile():
    """Six records on a 16 x 16 tile, none near a threshold: opacities well above 1/255 and below the clamp, no pixel stops."""
    rng = np.random.default_rng(3)
    L, Cn = 6, 5
    xy = rng.uniform(3, 13, (L, 2))
    s = rng.uniform(12.0, 16.0, L)
    rho = rng.uniform(-0.4, 0.4, L)
    cov = np.stack([s * s, rho * s * s * 0.8, 0.64 * s * s], 1)                 # (m00, m01, m11)
    det = cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2
    co = np.stack([cov[:, 2] / det, -cov[:, 1] / det, cov[:, 0] / det, rng.uniform(0.2, 0.45, L)], 1)
    return xy, co, cov, rng.normal(size=(L, Cn)), rng.uniform(-1, 1, Cn), rng.normal(size=(Cn, 16, 16))


def _loss(xy, co, feat, bg, g):
    return float((R.tile_backward(xy, co, feat, 0, 0, 16, 16, bg, g, f32_forward=False)["out"] * g).sum())


def test_gradients_against_finite_differences():
    xy, co, cov, feat, bg, g = _fd_tile()
    ref = R.tile_backward(xy, co, feat, 0, 0, 16, 16, bg, g, f32_forward=False)
    assert (ref["pixels"] == 256).all() and (ref["free_pixels"] == 256).all() and ref["final_t"].min() > 0.01
    h = 1e-6

    def fd(change):
        return (_loss(*change(+h)) - _loss(*change(-h))) / (2 * h)
    for i in range(len(xy)):
        for c in range(feat.shape[1]):
            def ch(e, i=i, c=c):
                f2 = feat.copy(); f2[i, c] += e
                return xy, co, f2, bg, g
            assert abs(fd(ch) - ref["d_chan"][i, c]) <= 1e-6 * ref["M_d_chan"][i, c] + 1e-9, ("d_chan", i, c)
        for j in range(2):
            def ch(e, i=i, j=j):
                x2 = xy.copy(); x2[i, j] += e
                return x2, co, feat, bg, g
            assert abs(fd(ch) - ref["d_mean"][i, j]) <= 1e-5 * ref["M_d_mean"][i, j] + 1e-9, ("d_mean", i, j)
        for j in range(3):
            def ch(e, i=i, j=j):
                c2 = co.copy(); c2[i, j] += e * 1e-2
                return xy, c2, feat, bg, g
            assert abs(fd(ch) / 1e-2 - ref["d_conic"][i, j]) <= 1e-5 * ref["M_d_conic"][i, j] + 1e-7, ("d_conic", i, j)

        def ch(e, i=i):
            c2 = co.copy(); c2[i, 3] += e
            return xy, c2, feat, bg, g
        assert abs(fd(ch) - ref["d_op"][i, 0]) <= 1e-6 * ref["M_d_op"][i, 0] + 1e-9, ("d_op", i)
        # cov2D: Sigma -> Sigma + e E for a symmetric E; dL = e sum(E * [[m00, m01], [m01, m11]])
        for j, E in enumerate(([[1, 0], [0, 0]], [[0, 1], [1, 0]], [[0, 0], [0, 1]])):
            def ch(e, i=i, E=np.asarray(E, np.float64)):
                S = np.array([[cov[i, 0], cov[i, 1]], [cov[i, 1], cov[i, 2]]]) + e * 1e2 * E
                K = np.linalg.inv(S)
                c2 = co.copy(); c2[i, :3] = (K[0, 0], K[0, 1], K[1, 1])
                return xy, c2, feat, bg, g
            want = ref["d_cov"][i, j] * (2.0 if j == 1 else 1.0)
            assert abs(fd(ch) / 1e2 - want) <= 1e-4 * 2.0 * ref["M_d_cov"][i, j] + 1e-10, ("d_cov", i, j)


# ---- 4. superposition: three channels are the oracle's; C channels are ceil(C / 3) oracle runs -------------------------
@pytest.mark.parametrize("name", ["tile-65-opaque", "edge", "clamp"])
def test_superposition_against_the_oracle_and_absgrads_signed(name):
    scene, cam = SCENES[name]
    st = state_of(name)
    W, H = cam.width, cam.height
    n = st["means2D"].shape[0]
    Cn = 2 * R.CHUNK + 1
    feat, bg, g = R.features_of(n, Cn), R.background_of(Cn), R.gradient_of(cam, Cn)
    ref = R.backward(st, feat, bg, g, W, H)
    pad = (-Cn) % 3
    fp, bp, gp = np.pad(feat, ((0, 0), (0, pad))), np.pad(bg, (0, pad)), np.pad(g, ((0, pad), (0, 0), (0, 0)))
    total = {k: 0.0 for k in ("signed", "d_conic", "d_cov", "d_op")}
    ranges = np.asarray(st["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    values = np.asarray(st["values"]).view(np.uint32).astype(np.int64)
    gx = (W + 15) // 16
    for c in range(0, Cn + pad, 3):
        part = dict(st)
        part["rgb"] = fp[:, c:c + 3]
        total["signed"] = total["signed"] + A.frame_absgrad(part, W, H, bp[c:c + 3], gp[c:c + 3])["signed"]
        acc = {k: np.zeros((n, d)) for k, d in (("d_conic", 3), ("d_cov", 3), ("d_op", 1))}
        for t in range(len(ranges)):
            a, b = ranges[t]
            ids = values[a:b] if b > a else values[0:0]
            tx, ty = t % gx, t // gx
            tg = np.zeros((3, 16, 16))
            ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
            tg[:, : yb - ya, : xb - xa] = gp[c:c + 3, ya:yb, xa:xb]
            res = B.blend_tile_backward(st["means2D"][ids], st["conicOpacity"][ids], fp[ids, c:c + 3], tx, ty, W, H, bp[c:c + 3], tg,
                                        f32_forward=True)
            np.add.at(acc["d_conic"], ids, res["d_conic"])
            np.add.at(acc["d_cov"], ids, res["d_cov"])
            np.add.at(acc["d_op"], ids, res["d_op"].reshape(-1, 1))
            if c == 0:
                _close(res["d_col"], R.tile_backward(st["means2D"][ids], st["conicOpacity"][ids], fp[ids, :3], tx, ty, W, H, bp[:3], tg)["d_chan"],
                       "d_col", 1e-11)
        for k in acc:
            total[k] = total[k] + acc[k]
    scale = lambda name_: 1e-9 * ref["M_" + name_] + 1e-300            # (sums of ceil(C/3) parts: rounding of the float64 additions)
    assert (np.abs(total["signed"] - ref["d_mean"]) <= scale("d_mean")).all()
    for k in ("d_conic", "d_cov", "d_op"):
        assert (np.abs(total[k] - ref[k]) <= scale(k)).all(), k


# ---- 5. blindness guards --------------------------------------------------------------------------------------------------
def test_the_scenes_hold_the_cases_the_gpu_file_names():
    for length in R.LIST_LENGTHS:
        for kind in ("faint", "opaque"):
            st = state_of(f"tile-{length}-{kind}")
            assert int(st["ranges"].reshape(-1, 2)[0, 1]) - int(st["ranges"].reshape(-1, 2)[0, 0]) == length
    assert int(np.asarray(state_of("tile-257-faint")["nContrib"]).max()) == 257          # lists crossing 64 and 256
    assert int(np.asarray(state_of("tile-65-faint")["nContrib"]).max()) == 65
    for name in ("tile-257-opaque", "edge", "clamp", "fill"):
        scene, cam = SCENES[name]
        st = state_of(name)
        fw = contrib_stopped(st, cam)
        assert fw >= 16, (name, fw)                                       # pixels stopped by the cut-off
    scene, cam = SCENES["clamp"]
    st = state_of("clamp")
    n = st["means2D"].shape[0]
    ref = R.backward(st, R.features_of(n, 3), None, R.gradient_of(cam, 3), cam.width, cam.height)
    partly = (ref["free_pixels"] > 0) & (ref["free_pixels"] < ref["pixels"])
    assert partly.sum() >= 12                                             # records clamped on some pixels and free on others
    assert (ref["pixels"] == 0).sum() >= 4 and (ref["pixels"] > 0).sum() >= 40
    # a chunk boundary inside C: every channel count the GPU file uses, and where its chunks end
    width = lambda c: R.NARROW if c <= R.NARROW else R.CHUNK
    assert R.CHANNELS == (1, 3, 7, 8, 9, 15, 16, 17, 33) and [(-(-c // width(c))) for c in R.CHANNELS] == [1, 1, 1, 1, 1, 1, 1, 2, 3]
    # a kernel that dropped the background's seed, or a chunk's share of dL/dalpha, is seen: the geometry sums of C = 17 differ
    # from those of its first 16 channels alone by more than ten bounds on most blended Gaussians
    st = state_of("edge")
    scene, cam = SCENES["edge"]
    n = st["means2D"].shape[0]
    feat, bg, g = R.features_of(n, 17), R.background_of(17), R.gradient_of(cam, 17)
    full = R.backward(st, feat, bg, g, cam.width, cam.height)
    head = R.backward(st, feat[:, :16], bg[:16], g[:16], cam.width, cam.height)
    seen = np.abs(full["d_mean"] - head["d_mean"]) > 10 * R.bound(full, "d_mean")
    assert seen.any(1)[full["free_pixels"] > 0].mean() >= 0.5
    nobg = R.backward(st, feat, None, g, cam.width, cam.height)
    seen = np.abs(full["d_mean"] - nobg["d_mean"]) > 10 * R.bound(full, "d_mean")
    assert seen.any(1)[full["free_pixels"] > 0].mean() >= 0.5


def contrib_stopped(st, cam):
    import contrib_ref
    return int(contrib_ref.of_state(st, cam)["stopped"].sum())


# ---- 6. ABI -----------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "gsrast_amd_features.h")).read()


def _declared_functions():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_features_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_features_backward", "gsr_features_forward", "gsr_features_temp_bytes"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_features.h but not exported"
    assert set(_capi.FEATURES_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES):
        assert not set(_capi.FEATURES_SIGNATURES) & set(other)
    defines = dict(re.findall(r"#define (GSR_FEATURES_[A-Z_]+) (\d+)", _header()))
    assert int(defines["GSR_FEATURES_MAX_CHANNELS"]) == _capi.GSR_FEATURES_MAX_CHANNELS == 256
    assert int(defines["GSR_FEATURES_CHUNK"]) == _capi.GSR_FEATURES_CHUNK == R.CHUNK
    assert int(defines["GSR_FEATURES_CHUNK_NARROW"]) == _capi.GSR_FEATURES_CHUNK_NARROW == R.NARROW
    assert L.gsr_features_temp_bytes(100, 17) == 8 * 100 * 17
    assert L.gsr_features_temp_bytes(100, 0) == 0 and L.gsr_features_temp_bytes(100, 257) == 0 and L.gsr_features_temp_bytes(0, 3) == 0


def test_the_struct_is_the_headers_and_the_header_compiles_as_c(tmp_path):
    names = [n for n, _ in _capi.FeaturesArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_features_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_features_args, {f}));' for f in names)
    src, exe = tmp_path / "features_abi.c", tmp_path / "features_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_features.h"\nint main(void){' + body
                   + "int (*fn)(gsr_features_args*) = gsr_features_forward; (void)fn; fn = gsr_features_backward; (void)fn; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "features_abi.o")])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_features.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.FeaturesArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.FeaturesArgs, f).offset, f


# ---- 7. the error contract, without a device --------------------------------------------------------------------------------
N, W, H, RENDERED, CH = 100, 40, 24, 500, 5
GEO, IMG, BIN, SCENE = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # addresses nothing dereferences: every case is decided before


def valid_args(keep):
    """gsr_features_args that pass every check of both calls (they would launch). keep: receives the two outputs and the scratch
    (ctypes holds addresses only), with a pattern no refused call may touch."""
    L = _capi.lib()
    bst = _capi.BinningState()
    L.gsr_binning_from_chunk(BIN, RENDERED, C.byref(bst))
    a = _capi.FeaturesArgs()
    a.struct_size = C.sizeof(_capi.FeaturesArgs)
    a.num_gaussians, a.width, a.height, a.channels = N, W, H, CH
    a.means2D, a.conic_opacity = GEO + 0x1000, GEO + 0x2000
    a.ranges, a.n_contrib, a.final_t = IMG, IMG + 0x1000, IMG + 0x3000
    a.point_list = bst.values
    a.features, a.background, a.dL_dout = SCENE, SCENE + 0x10000, SCENE + 0x20000
    r = a.receipt
    r.magic, r.plan_used = _capi.GSR_RECEIPT_MAGIC, 1
    r.num_gaussians, r.width, r.height, r.tile_row_begin, r.tile_row_end = N, W, H, 0, 2
    r.num_rendered, r.num_visible, r.serial = RENDERED, N, 0
    r.geometry_chunk, r.image_chunk, r.binning_chunk = GEO, IMG, BIN
    out, grad = (C.c_float * (CH * W * H))(*([7.0] * (CH * W * H))), (C.c_float * (N * CH))(*([7.0] * (N * CH)))
    sums, geo = (C.c_double * (N * CH + 1))(), (C.c_double * (12 * N + 1))()
    keep.extend([out, grad, sums, geo])
    a.out, a.dL_dfeatures, a.feature_sums_f64, a.geometry_sums_f64 = (C.addressof(v) for v in (out, grad, sums, geo))
    return a


def _set(path, value):
    def change(a):
        obj = a
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value)
    return change


def _odd(field, by=4):
    def change(a):
        setattr(a, field, getattr(a, field) + by)
    return change


BOTH, FORWARD, BACKWARD = ("gsr_features_forward", "gsr_features_backward"), ("gsr_features_forward",), ("gsr_features_backward",)
REFUSALS = {
    "struct_size too small": (BOTH, _set("struct_size", C.sizeof(_capi.FeaturesArgs) - 8)),
    "struct_size too large": (BOTH, _set("struct_size", C.sizeof(_capi.FeaturesArgs) + 8)),
    "struct_size zero": (BOTH, _set("struct_size", 0)),
    "no channels": (BOTH, _set("channels", 0)),
    "negative channels": (BOTH, _set("channels", -3)),
    "257 channels": (BOTH, _set("channels", 257)),
    "no receipt": (BOTH, _set("receipt.magic", 0)),
    "a receipt of something else": (BOTH, _set("receipt.magic", 0x12345678)),
    "another N": (BOTH, _set("num_gaussians", N + 1)),
    "no Gaussians": (BOTH, _set("num_gaussians", 0)),
    "another width": (BOTH, _set("width", W + 16)),
    "another height": (BOTH, _set("height", H + 16)),
    "the receipt's N": (BOTH, _set("receipt.num_gaussians", N - 1)),
    "rows the receipt does not have": (BOTH, _set("tile_row_end", 1)),
    "rows outside the frame": (BOTH, _set("tile_row_end", 3)),
    "point_list of another chunk": (BOTH, _set("point_list", BIN + 0x40)),
    "no point_list": (BOTH, _set("point_list", None)),
    "no binning chunk": (BOTH, _set("receipt.binning_chunk", None)),
    "sorted lists skipped": (BOTH, _set("receipt.plan_used", 2 | _capi.GSR_PLAN_LISTS_SKIPPED)),
    "no means2D": (BOTH, _set("means2D", None)),
    "no conic_opacity": (BOTH, _set("conic_opacity", None)),
    "no ranges": (BOTH, _set("ranges", None)),
    "no n_contrib": (BOTH, _set("n_contrib", None)),
    "no final_t": (BOTH, _set("final_t", None)),
    "no features": (BOTH, _set("features", None)),
    "means2D off an 8-byte boundary": (BOTH, _odd("means2D")),
    "conic_opacity off a 16-byte boundary": (BOTH, _odd("conic_opacity", 8)),
    "no out": (FORWARD, _set("out", None)),
    "no dL_dout": (BACKWARD, _set("dL_dout", None)),
    "no dL_dfeatures": (BACKWARD, _set("dL_dfeatures", None)),
    "no scratch": (BACKWARD, _set("feature_sums_f64", None)),
    "scratch off an 8-byte boundary": (BACKWARD, _odd("feature_sums_f64")),
    "geometry sums off an 8-byte boundary": (BACKWARD, _odd("geometry_sums_f64")),
}


def refused_untouched(case):
    L = _capi.lib()
    calls, change = REFUSALS[case]
    for name in calls:
        keep = []
        a = valid_args(keep)
        change(a)
        assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
        assert getattr(L, name)(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG, (case, name)
        assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""
        assert set(keep[0]) == {7.0} and set(keep[1]) == {7.0} and not any(keep[2]) and not any(keep[3])


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_decided_without_a_device(case):
    refused_untouched(case)


def test_null_args_are_refused():
    L = _capi.lib()
    for name in BOTH:
        assert getattr(L, name)(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
