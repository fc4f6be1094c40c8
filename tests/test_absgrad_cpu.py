"""CPU: the absolute screen-space gradient (gsr_absgrad, include/gsrast_amd_absgrad.h). The reference of tests/absgrad_ref.py
pinned to the project's oracle (oracle/backward_np.blend_tile_backward) for the colour term, its ordering |signed| <= A <= M, one
Gaussian on one pixel by hand, the blindness guards of the scenes tests/test_gpu_absgrad.py uses, the eighth header against its
ctypes table, every refusal of the call without a device, and DensityStats.update(absgrad=True) on a slot without the array."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import absgrad_ref as R
from helpers import ROOT
from oracle import backward_np as B
from oracle import cpu_oracle

from gsrast_amd import _capi

SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
JOINT_SCENES = ("edge", "clamp")          # the scenes the GPU file runs every combination of terms on


@functools.lru_cache(maxsize=None)
def state_of(name):
    scene, cam = SCENES[name]
    return cpu_oracle.forward(scene, cam)


@functools.lru_cache(maxsize=None)
def ref_of(name, terms="colour"):
    scene, cam = SCENES[name]
    return R.reference(state_of(name), scene, cam, terms)


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert (np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b))).all(), (what, float(np.abs(a - b).max()))


# ---- 1. pinned to the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_colour_only_is_the_oracles_d_mean_m_mean_and_k(name):
    scene, cam = SCENES[name]
    state = state_of(name)
    gc, _, _ = R.pixel_gradients(cam)
    W, H = cam.width, cam.height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    seen = 0
    for ty in range(gy):
        for tx in range(gx):
            a, b = (int(v) for v in state["ranges"][ty * gx + tx])
            ids = state["values"][a:b].astype(np.int64) if b > a else np.zeros(0, np.int64)
            tile_g = np.zeros((3, 16, 16))
            ya, yb, xa, xb = ty * 16, min(H, ty * 16 + 16), tx * 16, min(W, tx * 16 + 16)
            tile_g[:, : yb - ya, : xb - xa] = gc[:, ya:yb, xa:xb]
            args = (state["means2D"][ids], state["conicOpacity"][ids], state["rgb"][ids], tx, ty, W, H, R.BACKGROUND, tile_g)
            exp = B.blend_tile_backward(*args, f32_forward=True, magnitudes=True)
            got = R.tile_absgrad(*args)
            _close(got["signed"], exp["d_mean"], (name, tx, ty, "signed"))
            _close(got["M"], exp["M_mean"], (name, tx, ty, "M"))
            assert np.array_equal(got["k"], exp["k"]) and np.array_equal(got["pixels"], exp["pixels"])
            assert np.array_equal(got["free_pixels"], exp["free_pixels"])
            assert np.array_equal(got["n_contrib"], exp["n_contrib"]) and np.array_equal(got["final_t"], exp["final_t"])
            # ... and its forward is the C++ oracle's: the GPU's n_contrib and final_t are these, bit for bit
            assert np.array_equal(got["n_contrib"][: yb - ya, : xb - xa], state["nContrib"][ya:yb, xa:xb])
            assert np.array_equal(got["final_t"][: yb - ya, : xb - xa].astype(np.float32).view(np.uint32),
                                  state["finalT"][ya:yb, xa:xb].view(np.uint32))
            seen += int(got["pixels"].sum())
    assert seen > 0


# ---- 2. the ordering --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,terms", [(n, "colour") for n in SCENES] + [(n, t) for n in JOINT_SCENES for t in R.TERMS[1:]])
def test_signed_below_absolute_below_condition_scale(name, terms):
    ref = ref_of(name, terms)
    s, A, M = np.abs(ref["signed"]), ref["A"], ref["M"]
    assert (A >= 0).all() and (s <= A * (1 + 1e-12)).all() and (A <= M * (1 + 1e-12)).all()
    none = ref["pixels"] == 0
    assert (A[none] == 0).all() and (A[ref["free_pixels"] == 0] == 0).all()
    assert (A[ref["free_pixels"] > 0] > 0).all()       # (random gradients: a share cannot vanish)


# ---- 3. by hand -------------------------------------------------------------------------------------------------------------
def test_one_gaussian_on_one_pixel_by_hand():
    f = np.float32
    xy, co, col = np.array([[0.5, 0.25]], f), np.array([[0.5, 0.125, 0.75, 0.5]], f), np.array([[0.25, 0.5, 1.0]], f)
    bg, g = np.array([0.5, 0.25, 0.125]), np.array([1.0, -2.0, 0.5])
    tile_g = np.zeros((3, 16, 16))
    tile_g[:, 0, 0] = g
    ga = np.zeros((16, 16))
    ga[0, 0] = 0.375
    got = R.tile_absgrad(xy, co, col, 0, 0, 1, 1, bg, tile_g, ga)
    dx, dy = 0.5, 0.25
    power = f(-0.5) * ((f(0.5) * f(dx)) * f(dx) + (f(0.75) * f(dy)) * f(dy)) - (f(0.125) * f(dx)) * f(dy)
    G = float(cpu_oracle.expf(np.array([power], f))[0])
    alpha = float(f(0.5) * f(G))
    T_f = float(f(1.0) - f(alpha))                       # the forward's final transmittance; in front of the record T = 1
    cg = float(col[0].astype(np.float64) @ g)
    dL_dalpha = 1.0 * cg - T_f * (float(bg @ g) - 0.375) / (1.0 - alpha)
    dpow = 0.5 * G * dL_dalpha
    share = np.array([-(0.5 * dx + 0.125 * dy) * dpow, -(0.125 * dx + 0.75 * dy) * dpow])
    _close(got["signed"][0], share, "signed")
    _close(got["A"][0], np.abs(share), "A")
    assert got["k"].tolist() == [1] and got["pixels"].tolist() == [1] and got["free_pixels"].tolist() == [1]
    m_alpha = float(np.abs(col[0].astype(np.float64)) @ np.abs(g)) + T_f * (float(np.abs(bg) @ np.abs(g)) + 0.375) / (1.0 - alpha)
    _close(got["M"][0], np.array([(0.5 * dx + 0.125 * dy), (0.125 * dx + 0.75 * dy)]) * 0.5 * G * m_alpha, "M")
    # a clamped record (raw > 0.99) contributes nothing, on the same pixel
    co[0, 3] = 0.9999
    xy0 = np.array([[0.0, 0.0]], f)
    clamped = R.tile_absgrad(xy0, co, col, 0, 0, 1, 1, bg, tile_g)
    assert clamped["pixels"].tolist() == [1] and clamped["free_pixels"].tolist() == [0] and not clamped["A"].any()


# ---- 4. blindness guards ----------------------------------------------------------------------------------------------------
def test_the_scenes_tell_sum_of_abs_from_abs_of_sum():
    """On every scene with more than a handful of Gaussians at least 30 % of the blended, unclamped ones have A > 2 |signed| in
    some component (measured: 50 to 90 %): a kernel that took the absolute value of the sum would miss those by a factor of 2."""
    for name in SCENES:
        ref = ref_of(name)
        on = ref["free_pixels"] > 0
        if on.sum() < 20:
            continue
        far = (ref["A"][on] > 2.0 * np.abs(ref["signed"][on])).any(axis=1)
        print(f"{name}: {int(far.sum())} of {int(on.sum())} Gaussians with A > 2 |signed|")
        assert far.mean() >= 0.3, (name, float(far.mean()))
    assert (ref_of("fill")["pixels"][0] > 64 * 100)          # one splat over 64 tiles: 64 waves add into its row


@pytest.mark.parametrize("name", JOINT_SCENES)
def test_the_joint_result_is_not_the_sum_of_the_parts(name):
    """A(colour + depth) differs from A(colour) + A(depth) by more than ten times the GPU bound on at least half of the blended,
    unclamped Gaussians: a kernel that walked once per term and added would be caught. The same for colour + alpha."""
    scene, cam = SCENES[name]
    state = state_of(name)
    gc, gd, ga = R.pixel_gradients(cam)
    zero3 = np.zeros_like(gc)
    d = R.depth_values(scene["means3D"], cam.view)
    colour = ref_of(name)
    for terms, alone in (("colour+depth", R.frame_absgrad(state, cam.width, cam.height, R.BACKGROUND, zero3, gd, d)),
                         ("colour+alpha", R.frame_absgrad(state, cam.width, cam.height, R.BACKGROUND, zero3, None, None, ga))):
        joint = ref_of(name, terms)
        on = joint["free_pixels"] > 0
        gap = np.abs(colour["A"] + alone["A"] - joint["A"])
        assert (colour["A"] + alone["A"] >= joint["A"] * (1 - 1e-12)).all()
        told = (gap > 10.0 * R.bound(joint))[on].any(axis=1)
        print(f"{name} {terms}: {int(told.sum())} of {int(on.sum())} Gaussians tell joint from added")
        assert told.mean() >= 0.5, (name, terms, float(told.mean()))


def test_the_scenes_hold_the_cases_the_gpu_file_names():
    for length in R.LIST_LENGTHS:
        for kind in ("faint", "opaque"):
            state = state_of(f"tile-{length}-{kind}")
            assert int(state["ranges"][0, 1]) - int(state["ranges"][0, 0]) == length
    opaque = state_of("tile-257-opaque")
    early = opaque["nContrib"][opaque["nContrib"] < 257]
    assert early.size >= 100 and len(np.unique(early)) >= 4      # an opaque front ends pixels below the list length, at several depths
    assert int(state_of("tile-257-faint")["nContrib"].max()) == 257
    clamp = ref_of("clamp")
    partly = (clamp["free_pixels"] > 0) & (clamp["free_pixels"] < clamp["pixels"])
    clamped_pixels = int((clamp["pixels"] - clamp["free_pixels"]).sum())
    assert partly.sum() >= 12 and clamped_pixels >= 12, (int(partly.sum()), clamped_pixels)     # records with raw > 0.99: half of the 24 wide ones
    for name in ("edge", "clamp"):
        ref = ref_of(name)
        assert (ref["pixels"] == 0).sum() >= 4 and (ref["pixels"] > 0).sum() >= 40


# ---- 5. ABI -----------------------------------------------------------------------------------------------------------------
def _declared_functions():
    text = open(os.path.join(ROOT, "include", "gsrast_amd_absgrad.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_absgrad_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_absgrad"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_absgrad.h but not exported"
    assert set(_capi.ABSGRAD_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES):
        assert not set(_capi.ABSGRAD_SIGNATURES) & set(other)


def test_the_struct_is_the_headers_and_the_header_compiles_as_c(tmp_path):
    names = [n for n, _ in _capi.AbsgradArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_absgrad_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_absgrad_args, {f}));' for f in names)
    src, exe = tmp_path / "absgrad_abi.c", tmp_path / "absgrad_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_absgrad.h"\nint main(void){' + body
                   + "int (*fn)(gsr_absgrad_args*) = gsr_absgrad; (void)fn; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "absgrad_abi.o")])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_absgrad.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.AbsgradArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.AbsgradArgs, f).offset, f


# ---- 6. the error contract, without a device --------------------------------------------------------------------------------
N, W, H, RENDERED = 100, 40, 24, 500
GEO, IMG, BIN, SCENE = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # addresses nothing dereferences: every case is decided before


def valid_args(keep):
    """(gsr_absgrad_args, its gsr_backward_args) that pass every check (the call would launch). keep: receives the output and
    the scratch (ctypes holds addresses only), both with a pattern no refused call may touch."""
    L = _capi.lib()
    bst = _capi.BinningState()
    L.gsr_binning_from_chunk(BIN, RENDERED, C.byref(bst))
    b = _capi.BackwardArgs()
    b.struct_size = C.sizeof(_capi.BackwardArgs)
    b.num_gaussians, b.width, b.height = N, W, H
    b.background = SCENE
    b.means2D, b.conic_opacity, b.colors = GEO + 0x1000, GEO + 0x2000, GEO + 0x3000
    b.ranges, b.n_contrib, b.final_t = IMG, IMG + 0x1000, IMG + 0x3000
    b.point_list = bst.values
    b.dL_dout_color = SCENE + 0x1000
    r = b.receipt
    r.magic, r.plan_used = _capi.GSR_RECEIPT_MAGIC, 1
    r.num_gaussians, r.width, r.height, r.tile_row_begin, r.tile_row_end = N, W, H, 0, 2
    r.num_rendered, r.num_visible, r.serial = RENDERED, N, 0
    r.geometry_chunk, r.image_chunk, r.binning_chunk = GEO, IMG, BIN
    out, sums = (C.c_float * (2 * N))(*([7.0] * (2 * N))), (C.c_double * (2 * N + 1))()
    keep.extend([b, out, sums])
    a = _capi.AbsgradArgs()
    a.struct_size = C.sizeof(_capi.AbsgradArgs)
    a.backward = C.pointer(b)
    a.abs_dL_dmean2D, a.sums_f64 = C.addressof(out), C.addressof(sums)
    return a, b


def _set(path, value, on="a"):
    def change(a, b):
        obj = a if on == "a" else b
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value)
    return change


def _null_backward(a, b):
    a.backward = None


def _depth_without(which):
    def change(a, b):
        b.dL_dout_depth, b.means3D, b.view_matrix = SCENE + 0x2000, SCENE + 0x3000, SCENE + 0x4000
        setattr(b, which, None)
    return change


def _odd_scratch(a, b):
    a.sums_f64 = a.sums_f64 + 4


def _odd_output(a, b):
    a.abs_dL_dmean2D = a.abs_dL_dmean2D + 4


REFUSALS = {
    "struct_size too small": _set("struct_size", C.sizeof(_capi.AbsgradArgs) - 8),
    "struct_size too large": _set("struct_size", C.sizeof(_capi.AbsgradArgs) + 8),
    "struct_size zero": _set("struct_size", 0),
    "no backward struct": _null_backward,
    "the backward struct's size": _set("struct_size", C.sizeof(_capi.BackwardArgs) - 8, on="b"),
    "the backward struct's size zero": _set("struct_size", 0, on="b"),
    "no receipt": _set("receipt.magic", 0, on="b"),
    "a receipt of something else": _set("receipt.magic", 0x12345678, on="b"),
    "another N": _set("num_gaussians", N + 1, on="b"),
    "another width": _set("width", W + 16, on="b"),
    "another height": _set("height", H + 16, on="b"),
    "the receipt's N": _set("receipt.num_gaussians", N - 1, on="b"),
    "rows the receipt does not have": _set("tile_row_end", 1, on="b"),
    "rows outside the frame": _set("tile_row_end", 3, on="b"),
    "point_list of another chunk": _set("point_list", BIN + 0x40, on="b"),
    "no point_list": _set("point_list", None, on="b"),
    "no binning chunk": _set("receipt.binning_chunk", None, on="b"),
    "sorted lists skipped": _set("receipt.plan_used", 2 | _capi.GSR_PLAN_LISTS_SKIPPED, on="b"),
    "no background": _set("background", None, on="b"),
    "no means2D": _set("means2D", None, on="b"),
    "no conic_opacity": _set("conic_opacity", None, on="b"),
    "no colors": _set("colors", None, on="b"),
    "no ranges": _set("ranges", None, on="b"),
    "no n_contrib": _set("n_contrib", None, on="b"),
    "no final_t": _set("final_t", None, on="b"),
    "no dL_dout_color": _set("dL_dout_color", None, on="b"),
    "dL_dout_depth without means3D": _depth_without("means3D"),
    "dL_dout_depth without view_matrix": _depth_without("view_matrix"),
    "no output": _set("abs_dL_dmean2D", None),
    "no scratch": _set("sums_f64", None),
    "scratch off an 8-byte boundary": _odd_scratch,
    "output off an 8-byte boundary": _odd_output,
}


def refused_untouched(case):
    L = _capi.lib()
    keep = []
    a, b = valid_args(keep)
    REFUSALS[case](a, b)
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert L.gsr_absgrad(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""
    assert list(keep[1]) == [7.0] * (2 * N) and not any(keep[2])


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_decided_without_a_device(case):
    refused_untouched(case)


def test_null_args_are_refused():
    L = _capi.lib()
    assert L.gsr_absgrad(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG


# ---- 7. the statistics ------------------------------------------------------------------------------------------------------
def test_density_stats_refuses_a_slot_without_the_array():
    import torch
    from gsrast_amd.autograd import FrameSlot
    from gsrast_amd.densify import DensityStats
    assert FrameSlot().absgrad is False and FrameSlot(absgrad=True).absgrad is True
    stats = DensityStats(4, "cpu")
    slot = FrameSlot(absgrad=True)
    slot.radii = torch.zeros(4, dtype=torch.int32)
    slot.dL_dmean2D = torch.zeros((4, 2))
    assert slot.abs_dL_dmean2D is None
    with pytest.raises(ValueError, match="abs_dL_dmean2D"):
        stats.update(slot, 16, 16, absgrad=True)
    assert not stats.grad_accum.any() and not stats.denom.any()
