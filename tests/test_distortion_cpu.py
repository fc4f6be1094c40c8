"""CPU: the depth distortion map (gsr_distortion_forward / gsr_distortion_backward, include/gsrast_amd_distortion.h). The float64
walk of tests/distortion_ref.py against the brute-force double sum over pairs; its gradients against central finite differences
of the float64 forward; the float32 restatement of the header against it, forward and backward, under the rule the GPU file
applies; a blindness guard of that rule; the tenth header against its ctypes table; every refusal of the calls without a device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import distortion_ref as R
from helpers import BW_ATOL, BW_C, BW_TAU, ROOT
from oracle import cpu_oracle

from gsrast_amd import _capi

SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
KINDS = ("depth", "random")


@functools.lru_cache(maxsize=None)
def state_of(name):
    scene, cam = SCENES[name]
    return cpu_oracle.forward(scene, cam, background=R.A.BACKGROUND)


def values_of(name, kind):
    scene, cam = SCENES[name]
    return R.depth_values(scene, cam) if kind == "depth" else R.random_values(scene["means3D"].shape[0])


@functools.lru_cache(maxsize=None)
def forward_of(name, kind, power):
    scene, cam = SCENES[name]
    return R.forward32(state_of(name), values_of(name, kind), power, cam.width, cam.height)


@functools.lru_cache(maxsize=None)
def walk_of(name, kind, power, **kw):
    scene, cam = SCENES[name]
    return R.frame_walk(state_of(name), values_of(name, kind), power, R.gradient_of(cam), cam.width, cam.height,
                        moments=forward_of(name, kind, power)["moments"], **kw)


def _tiles(name):
    """(tx, ty, ids) of every tile of a scene's frame."""
    scene, cam = SCENES[name]
    st = state_of(name)
    ranges = np.asarray(st["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    lists = np.asarray(st["values"]).view(np.uint32).astype(np.int64)
    gx = (cam.width + 15) // 16
    for t, (a, b) in enumerate(ranges):
        yield t % gx, t // gx, (lists[a:b] if b > a else lists[0:0])


# ---- 1. the float64 forward is the double sum over pairs -----------------------------------------------------------------------
@pytest.mark.parametrize("power", R.POWERS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_float64_forward_against_the_brute_force_double_sum(name, kind, power):
    scene, cam = SCENES[name]
    st = state_of(name)
    vals = values_of(name, kind).astype(np.float64)
    seen = 0
    for tx, ty, ids in _tiles(name):
        if len(ids) == 0:
            continue
        res = R.tile_walk(st["means2D"][ids], st["conicOpacity"][ids], vals[ids], tx, ty, cam.width, cam.height, power, np.zeros((16, 16)),
                          f32_forward=False)      # (1 - T is the sum of the weights in front only where T is exact)
        w, m = res["w"], vals[ids]
        diff = m[:, None] - m[None, :]
        if power == 1 and kind == "depth":
            # The signed form is the absolute one only where the values do not decrease along the list: asserted, not assumed.
            # The lists are sorted by the geometry chunk's depths — under this profile the NDC z in float32, in which view
            # depths 3e-5 apart tie at a distance of 5, so the view depth itself decreases along two of these lists (by 3.0e-5
            # in tile-255-faint and 6.7e-6 in tile-256-opaque). The absolute form is therefore compared on the depth the frame
            # sorted by; the view depth is compared with its signed sum, below, like any other value.
            key = np.asarray(st["depths"], np.float64).reshape(-1)[ids]
            assert (np.diff(key) >= 0).all(), (name, "the frame's depth decreases along a list")
            sres = R.tile_walk(st["means2D"][ids], st["conicOpacity"][ids], key, tx, ty, cam.width, cam.height, 1, np.zeros((16, 16)),
                               f32_forward=False)
            absolute = (w * (np.abs(key[:, None] - key[None, :]) @ w)).sum(axis=0).reshape(16, 16)
            assert (np.abs(sres["out"] - absolute) <= 1e-12 * sres["M_out"] + 1e-300).all(), (name, "absolute", tx, ty)
            # (where the view depth is in order too, its signed form is the absolute one as well)
            if (np.diff(m) >= 0).all():
                assert (np.abs(res["out"] - (w * (np.abs(diff) @ w)).sum(axis=0).reshape(16, 16)) <= 1e-12 * res["M_out"] + 1e-300).all()
        if power == 1:
            pair = np.where(np.arange(len(m))[:, None] > np.arange(len(m))[None, :], diff, -diff)      # signed in list order
        else:
            pair = diff * diff
        brute = (w * (pair @ w)).sum(axis=0).reshape(16, 16)
        assert (np.abs(res["out"] - brute) <= 1e-12 * res["M_out"] + 1e-300).all(), (name, kind, power, tx, ty)
        seen += int((res["blended"] >= 2).sum())
    assert seen > 0 or name.startswith("tile-1-")


def test_the_signed_form_is_not_the_absolute_one_for_values_in_no_order():
    """(why the header says `signed`: with random values the two differ, so the test above compares each with its own sum)"""
    name = "tile-65-faint"
    scene, cam = SCENES[name]
    st = state_of(name)
    vals = values_of(name, "random").astype(np.float64)
    (tx, ty, ids), = list(_tiles(name))
    res = R.tile_walk(st["means2D"][ids], st["conicOpacity"][ids], vals[ids], tx, ty, cam.width, cam.height, 1, np.zeros((16, 16)), f32_forward=False)
    m = vals[ids]
    absolute = (res["w"] * (np.abs(m[:, None] - m[None, :]) @ res["w"])).sum(axis=0).reshape(16, 16)
    assert (np.abs(res["out"] - absolute) > 1e-3 * absolute)[res["blended"] >= 2].any()


# ---- 2. gradients against central finite differences of the float64 forward ------------------------------------------------
def _fd_tile():
    """Six records on a 16 x 16 tile, none near a threshold (tests/test_features_cpu.py's tile), with values of either sign."""
    rng = np.random.default_rng(3)
    L = 6
    xy = rng.uniform(3, 13, (L, 2))
    s = rng.uniform(12.0, 16.0, L)
    rho = rng.uniform(-0.4, 0.4, L)
    cov = np.stack([s * s, rho * s * s * 0.8, 0.64 * s * s], 1)
    det = cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2
    co = np.stack([cov[:, 2] / det, -cov[:, 1] / det, cov[:, 0] / det, rng.uniform(0.2, 0.45, L)], 1)
    return xy, co, rng.normal(size=L), rng.normal(size=(16, 16))


def _loss(xy, co, vals, g, power):
    return float((R.tile_walk(xy, co, vals, 0, 0, 16, 16, power, g, f32_forward=False)["out"] * g).sum())


@pytest.mark.parametrize("power", R.POWERS)
def test_gradients_against_finite_differences(power):
    xy, co, vals, g = _fd_tile()
    ref = R.tile_walk(xy, co, vals, 0, 0, 16, 16, power, g, f32_forward=False)
    assert (ref["pixels"] == 256).all() and (ref["free_pixels"] == 256).all() and ref["final_t"].min() > 0.01
    h = 1e-6

    def fd(change):
        return (_loss(*change(+h), power) - _loss(*change(-h), power)) / (2 * h)
    for i in range(len(xy)):
        def ch(e, i=i):
            v2 = vals.copy(); v2[i] += e
            return xy, co, v2, g
        assert abs(fd(ch) - ref["d_val"][i, 0]) <= 1e-6 * ref["M_d_val"][i, 0] + 1e-9, ("d_val", i)

        def ch(e, i=i):                           # (alpha = opacity x G: the opacity's gradient is sum G dL/dalpha)
            c2 = co.copy(); c2[i, 3] += e
            return xy, c2, vals, g
        assert abs(fd(ch) - ref["d_op"][i, 0]) <= 1e-6 * ref["M_d_op"][i, 0] + 1e-9, ("d_op", i)
        for j in range(2):
            def ch(e, i=i, j=j):
                x2 = xy.copy(); x2[i, j] += e
                return x2, co, vals, g
            assert abs(fd(ch) - ref["d_mean"][i, j]) <= 1e-5 * ref["M_d_mean"][i, j] + 1e-9, ("d_mean", i, j)
        for j in range(3):
            def ch(e, i=i, j=j):
                c2 = co.copy(); c2[i, j] += e * 1e-2
                return xy, c2, vals, g
            assert abs(fd(ch) / 1e-2 - ref["d_conic"][i, j]) <= 1e-5 * ref["M_d_conic"][i, j] + 1e-7, ("d_conic", i, j)
    # the value gradients of a pixel add up to nothing: out does not move with a common shift (nor with m0)
    assert abs(ref["d_val"].sum()) <= 1e-12 * ref["M_d_val"].sum()
    shifted = _loss(xy, co, vals + 3.0, g, power)
    assert abs(shifted - _loss(xy, co, vals, g, power)) <= 1e-11 * abs(shifted) + 1e-12


# ---- 3. the float32 restatement against float64 ------------------------------------------------------------------------------
@pytest.mark.parametrize("power", R.POWERS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(SCENES))
def test_float32_restatement_against_float64(name, kind, power):
    scene, cam = SCENES[name]
    st, fw, ref = state_of(name), forward_of(name, kind, power), walk_of(name, kind, power)
    assert np.array_equal(fw["nContrib"], np.asarray(st["nContrib"]).view(np.uint32).reshape(fw["nContrib"].shape)), "nContrib"
    assert np.array_equal(fw["finalT"].view(np.uint32), np.asarray(st["finalT"], np.float32).view(np.uint32).reshape(fw["finalT"].shape)), "finalT"
    assert np.array_equal(fw["blended"], ref["blended"])
    # forward: per pixel, n the records it blended
    err = np.abs(fw["out"].astype(np.float64) - ref["out"])
    assert (err <= BW_TAU * (ref["blended"] + BW_C) * ref["M_out"] + BW_ATOL).all(), (name, kind, power, float(err.max()))
    none = ref["blended"] == 0
    assert (fw["out"][none] == 0).all() and (fw["moments"][:, none] == 0).all()
    if power == 1:
        assert (fw["moments"][2] == 0).all()
    # backward: the header's lines in float32 against the same lines in float64
    lines = walk_of(name, kind, power, f32_lines=True)
    for key, _ in R.SUMS:
        over = np.abs(lines[key] - ref[key]) > R.bound(ref, key)
        assert not over.any(), (name, kind, power, key, R.worst_ratio(lines[key], ref, key))


# ---- 4. a blindness guard -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("power", R.POWERS)
@pytest.mark.parametrize("name", list(SCENES))
def test_a_walk_without_its_suffix_term_is_seen(name, power):
    """dL/dalpha without S inv: every scene with two records in some pixel has a Gaussian outside the bound."""
    ref = walk_of(name, "depth", power)
    if int(ref["blended"].max()) < 2:
        assert name.startswith("tile-1-")
        return
    blind = walk_of(name, "depth", power, drop_suffix=True)
    outside = [bool((np.abs(blind[key] - ref[key]) > R.bound(ref, key)).any()) for key in ("d_mean", "d_conic", "d_op", "d_cov")]
    assert all(outside), (name, power, outside)
    assert np.array_equal(blind["d_val"], ref["d_val"])


# ---- 5. ABI ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "gsrast_amd_distortion.h")).read()


def test_library_exports_every_symbol_the_distortion_header_declares():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))
    assert names == ["gsr_distortion_backward", "gsr_distortion_forward", "gsr_distortion_temp_bytes"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_distortion.h but not exported"
    assert set(_capi.DISTORTION_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES):
        assert not set(_capi.DISTORTION_SIGNATURES) & set(other)
    assert L.gsr_distortion_temp_bytes(100) == 800 and L.gsr_distortion_temp_bytes(0) == 0 and L.gsr_distortion_temp_bytes(-4) == 0


def test_the_struct_is_the_headers_and_the_header_compiles_as_c(tmp_path):
    names = [n for n, _ in _capi.DistortionArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_distortion_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_distortion_args, {f}));' for f in names)
    src, exe = tmp_path / "distortion_abi.c", tmp_path / "distortion_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_distortion.h"\nint main(void){' + body
                   + "int (*fn)(gsr_distortion_args*) = gsr_distortion_forward; (void)fn; fn = gsr_distortion_backward; (void)fn; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "distortion_abi.o")])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_distortion.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.DistortionArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.DistortionArgs, f).offset, f


# ---- 6. the error contract, without a device ------------------------------------------------------------------------------------
N, W, H, RENDERED = 100, 40, 24, 500
GEO, IMG, BIN, SCENE = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # addresses nothing dereferences: every case is decided before


def valid_args(keep):
    """gsr_distortion_args that pass every check of both calls (they would launch). keep: receives the outputs and the scratches
    (ctypes holds addresses only), with a pattern no refused call may touch."""
    L = _capi.lib()
    bst = _capi.BinningState()
    L.gsr_binning_from_chunk(BIN, RENDERED, C.byref(bst))
    a = _capi.DistortionArgs()
    a.struct_size = C.sizeof(_capi.DistortionArgs)
    a.num_gaussians, a.width, a.height, a.power = N, W, H, 2
    a.means2D, a.conic_opacity = GEO + 0x1000, GEO + 0x2000
    a.ranges, a.n_contrib, a.final_t = IMG, IMG + 0x1000, IMG + 0x3000
    a.point_list = bst.values
    a.values, a.dL_dout = SCENE, SCENE + 0x20000
    r = a.receipt
    r.magic, r.plan_used = _capi.GSR_RECEIPT_MAGIC, 1
    r.num_gaussians, r.width, r.height, r.tile_row_begin, r.tile_row_end = N, W, H, 0, 2
    r.num_rendered, r.num_visible, r.serial = RENDERED, N, 0
    r.geometry_chunk, r.image_chunk, r.binning_chunk = GEO, IMG, BIN
    out, mom, grad = (C.c_float * (W * H))(*([7.0] * (W * H))), (C.c_float * (3 * W * H))(*([7.0] * (3 * W * H))), (C.c_float * N)(*([7.0] * N))
    sums, geo = (C.c_double * (N + 1))(), (C.c_double * (12 * N + 1))()
    keep.extend([out, mom, grad, sums, geo])
    a.out, a.moments, a.dL_dvalues, a.value_sums_f64, a.geometry_sums_f64 = (C.addressof(v) for v in (out, mom, grad, sums, geo))
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


BOTH, FORWARD, BACKWARD = ("gsr_distortion_forward", "gsr_distortion_backward"), ("gsr_distortion_forward",), ("gsr_distortion_backward",)
REFUSALS = {
    "struct_size too small": (BOTH, _set("struct_size", C.sizeof(_capi.DistortionArgs) - 8)),
    "struct_size too large": (BOTH, _set("struct_size", C.sizeof(_capi.DistortionArgs) + 8)),
    "struct_size zero": (BOTH, _set("struct_size", 0)),
    "power 0": (BOTH, _set("power", 0)),
    "power 3": (BOTH, _set("power", 3)),
    "power -1": (BOTH, _set("power", -1)),
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
    "no values": (BOTH, _set("values", None)),
    "no moments": (BOTH, _set("moments", None)),
    "means2D off an 8-byte boundary": (BOTH, _odd("means2D")),
    "ranges off an 8-byte boundary": (BOTH, _odd("ranges")),
    "conic_opacity off a 16-byte boundary": (BOTH, _odd("conic_opacity", 8)),
    "no out": (FORWARD, _set("out", None)),
    "no dL_dout": (BACKWARD, _set("dL_dout", None)),
    "no dL_dvalues": (BACKWARD, _set("dL_dvalues", None)),
    "no scratch": (BACKWARD, _set("value_sums_f64", None)),
    "scratch off an 8-byte boundary": (BACKWARD, _odd("value_sums_f64")),
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
        assert all(set(v) == {7.0} for v in keep[:3]) and not any(keep[3]) and not any(keep[4])


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_decided_without_a_device(case):
    refused_untouched(case)


def test_null_args_are_refused():
    L = _capi.lib()
    for name in BOTH:
        assert getattr(L, name)(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
