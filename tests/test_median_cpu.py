"""CPU: the median map and the per-pixel Gaussian ids (gsr_median_forward / gsr_median_backward, include/gsrast_amd_median.h).
The float32 restatement of tests/median_ref.py by hand on a three-record pixel, against cpu_oracle.forward (its finalT /
nContrib bit for bit on every scene tests/test_gpu_median.py uses: what the GPU comparison rests on), against contrib_ref's
`dominant` and against the forward's own last contributor; the scenes' blindness guards; the float64 backward by hand; the twelfth
header against its ctypes table; every refusal of the calls without a device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import contrib_ref
import median_ref as R
from helpers import ROOT
from oracle import cpu_oracle

from gsrast_amd import _capi

SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
NONE = int(R.NONE)


@functools.lru_cache(maxsize=None)
def state_of(name):
    scene, cam = SCENES[name]
    return cpu_oracle.forward(scene, cam)


@functools.lru_cache(maxsize=None)
def forward_of(name, threshold):
    scene, cam = SCENES[name]
    return R.of_state(state_of(name), cam, R.depth_values(scene["means3D"], cam.view), threshold)


# ---- 1. the reference by hand -------------------------------------------------------------------------------------------------
def _stack(opacities, values, threshold, w=1, h=1):
    """Round Gaussians centred on pixel (0, 0), front to back in the order given: there power = 0 and alpha = min(0.99, opacity)."""
    n = len(opacities)
    co = np.stack([np.full(n, 0.5), np.zeros(n), np.full(n, 0.5), np.asarray(opacities)], 1).astype(np.float32)
    return R.forward(np.zeros((n, 2), np.float32), co, np.array([[0, n]], np.uint32), np.arange(n, dtype=np.uint32),
                     None if values is None else np.asarray(values, np.float32), w, h, threshold)


def test_three_records_over_one_pixel_by_hand():
    # alpha 0.4 three times: T in front of the records is 1, 0.6, 0.36, the weights 0.4, 0.24, 0.144
    vals = [10.0, 20.0, 30.0]
    for threshold, want in ((0.5, 1), (0.05, 2), (0.0, 2), (R.FIRST_HIT, 0), (0.6, 0), (0.36, 1), (0.35, 2)):
        got = _stack([0.4, 0.4, 0.4], vals, threshold)
        # (0.6 and 0.36: T > threshold is strict; float32 1 - 0.4f is just above 0.6f's neighbour below — stated from the bits)
        t1 = np.float32(1.0) * (np.float32(1.0) - np.float32(0.4))
        t2 = t1 * (np.float32(1.0) - np.float32(0.4))
        by_hand = max(i for i, t in enumerate((np.float32(1.0), t1, t2)) if t > np.float32(threshold))
        assert by_hand == want, (threshold, by_hand, want)
        assert got["ids"][0, 0] == want and got["out"][0, 0] == np.float32(vals[want]), threshold
        assert got["dominant_ids"][0, 0] == 0 and got["nContrib"][0, 0] == 3 and got["blended"][0, 0] == 3
        assert got["sel_pos"][0, 0] == want + 1 and got["first_pos"][0, 0] == 1 and got["last_pos"][0, 0] == 3
    # the heaviest record behind: 0.1, then 0.9 of the 0.9 left
    assert _stack([0.1, 0.9, 0.5], vals, 0.5)["dominant_ids"][0, 0] == 1
    # a tie for dominant stays in front (contrib_ref's case): 0.2, then 0.25 of 0.8 rounds to 0.2f again
    assert _stack([0.2, 0.25, 0.1], vals, 0.5)["dominant_ids"][0, 0] == 0
    # below 1/255: blended by nobody — NONE, and 0.0 in the map; without values the map stays zero
    none = _stack([0.003], [5.0], 0.5)
    assert none["ids"][0, 0] == NONE and none["dominant_ids"][0, 0] == NONE and none["out"][0, 0] == 0 and none["blended"][0, 0] == 0
    assert _stack([0.4], None, 0.5)["out"][0, 0] == 0
    # 0.5, then two at 0.99: the third is the record the pixel stops ON, which is not blended: the last blended record is the second
    stop = _stack([0.5, 1.0, 1.0], vals, 0.0)
    assert stop["ids"][0, 0] == 1 and stop["nContrib"][0, 0] == 2 and stop["out"][0, 0] == np.float32(20.0)
    # a pixel whose transmittance never crosses keeps its last blended record (RaDe-GS masks it by !(final_t > threshold))
    faint = _stack([0.1, 0.1], vals, 0.5)
    assert faint["ids"][0, 0] == 1 and faint["finalT"][0, 0] > 0.5
    # a faint record between two: the skipped one does not count
    assert _stack([0.3, 0.003, 0.3], vals, 0.0)["ids"][0, 0] == 2 and _stack([0.3, 0.003, 0.3], vals, 0.0)["blended"][0, 0] == 2


def test_the_float64_backward_by_hand():
    ids = np.array([[0, 2, 2], [NONE, 7, 0]], np.uint32)
    g = np.array([[1.0, 0.5, 0.25], [100.0, 100.0, -3.0]], np.float32)
    sums, mags, pixels = R.backward(ids, g, 3)
    assert sums.tolist() == [-2.0, 0.0, 0.75] and mags.tolist() == [4.0, 0.0, 0.75] and pixels.tolist() == [2, 0, 2]
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.75) == 2.0 ** -24
    g = R.exact_gradient(SCENES["edge"][1])
    assert np.array_equal(np.round(g.astype(np.float64) * 1024) / 1024, g.astype(np.float64)) and np.abs(g).max() <= 1 and len(np.unique(g)) > 300


# ---- 2. against the oracle, contrib_ref and the forward's own outputs -------------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_reference_forward_is_the_oracles_bit_for_bit(name):
    """The allowed mismatch is 0: the GPU's finalT / nContrib are the oracle's bit for bit (tests/test_gpu_parity.py), so the
    replay's alpha, T and decisions are the GPU's."""
    state = state_of(name)
    for threshold in R.THRESHOLDS:
        ref = forward_of(name, threshold)
        assert np.array_equal(ref["finalT"].view(np.uint32), np.asarray(state["finalT"], np.float32).view(np.uint32).reshape(ref["finalT"].shape))
        assert np.array_equal(ref["nContrib"], np.asarray(state["nContrib"]).view(np.uint32).reshape(ref["nContrib"].shape))
        assert np.array_equal(ref["last_pos"], ref["nContrib"]) and ((ref["ids"] != R.NONE) == (ref["nContrib"] > 0)).all()
        assert ((ref["dominant_ids"] != R.NONE) == (ref["nContrib"] > 0)).all()


@pytest.mark.parametrize("name", list(SCENES))
def test_the_histogram_of_dominant_ids_is_contrib_refs_dominant(name):
    scene, cam = SCENES[name]
    ref = forward_of(name, 0.5)
    n = scene["means3D"].shape[0]
    dom = ref["dominant_ids"]
    hist = np.bincount(dom[dom != R.NONE].astype(np.int64), minlength=n).astype(np.uint64)
    want = contrib_ref.of_state(state_of(name), cam)["dominant"]
    assert np.array_equal(hist, want)
    for threshold in R.THRESHOLDS:             # (the dominant decision does not look at the threshold)
        assert np.array_equal(forward_of(name, threshold)["dominant_ids"], dom)


@pytest.mark.parametrize("name", list(SCENES))
def test_threshold_zero_selects_the_last_contributor(name):
    scene, cam = SCENES[name]
    st, ref = state_of(name), forward_of(name, 0.0)
    ranges = np.asarray(st["ranges"]).view(np.uint32).reshape(-1, 2).astype(np.int64)
    lists = np.asarray(st["values"]).view(np.uint32)
    gx = (cam.width + 15) // 16
    ys, xs = np.nonzero(ref["nContrib"] > 0)
    assert len(ys) > 0
    tile = (ys // 16) * gx + xs // 16
    assert np.array_equal(ref["ids"][ys, xs], lists[ranges[tile, 0] + ref["nContrib"][ys, xs].astype(np.int64) - 1])
    # ... and just under 1 the first blended record
    first = forward_of(name, R.FIRST_HIT)
    assert np.array_equal(first["sel_pos"], first["first_pos"])
    assert np.array_equal(first["ids"][ys, xs], lists[ranges[tile, 0] + first["first_pos"][ys, xs] - 1])
    # the map is the gather
    vals = R.depth_values(scene["means3D"], cam.view)
    assert np.array_equal(ref["out"][ys, xs].view(np.uint32), vals[ref["ids"][ys, xs]].view(np.uint32)) and (ref["out"][ref["nContrib"] == 0] == 0).all()


# ---- 3. blindness guards ------------------------------------------------------------------------------------------------------------
def _inner(ref):
    """Pixels that blended something and selected a record that is neither their first nor their last blended one."""
    return (ref["blended"] > 0) & (ref["sel_pos"] != ref["first_pos"]) & (ref["sel_pos"] != ref["last_pos"])


@pytest.mark.parametrize("name", [f"tile-{L}-opaque" for L in R.LIST_LENGTHS if L >= 63] + ["edge"])
def test_the_median_is_neither_the_first_nor_the_last_record_for_half_the_pixels(name):
    """Measured here: 179-231 of 256 on the one-tile scenes, 639 of 843 on `edge`. A walk that returned the first hit or the last
    contributor for the median would be seen."""
    ref = forward_of(name, 0.5)
    inner, blended = int(_inner(ref).sum()), int((ref["blended"] > 0).sum())
    print(f"[median guard] {name}: {inner} of {blended}")
    assert 2 * inner >= blended > 0, (name, inner, blended)


def test_the_fill_scene_has_a_thousand_such_pixels():
    ref = forward_of("fill", 0.5)
    inner = int(_inner(ref).sum())
    print(f"[median guard] fill: {inner}")
    assert inner >= 1000


@pytest.mark.parametrize("name", ["tile-257-opaque", "tile-600-opaque"])
def test_deep_selections_beyond_one_batch_and_one_round(name):
    """At threshold 0.05 a pixel's selection sits deep in the list: beyond the wave's first batch of 64 and beyond position 256.
    Measured here: 23 / 126 and 86 / 156."""
    ref = forward_of(name, 0.05)
    deep, far = int((ref["sel_pos"] > 256).sum()), int((ref["sel_pos"] > 64).sum())
    print(f"[median guard] {name}: {deep} beyond 256, {far} beyond 64")
    assert deep >= 10 and far >= 100, (name, deep, far)


# ---- 4. ABI ---------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "gsrast_amd_median.h")).read()


def test_library_exports_every_symbol_the_median_header_declares():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))
    assert names == ["gsr_median_backward", "gsr_median_forward", "gsr_median_temp_bytes"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_median.h but not exported"
    assert set(_capi.MEDIAN_SIGNATURES) == set(names), "ctypes table and header disagree"
    others = (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
              _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES,
              _capi.DISTORTION_SIGNATURES, _capi.NORMALS_SIGNATURES)
    assert len(others) == 11
    for other in others:
        assert not set(_capi.MEDIAN_SIGNATURES) & set(other)
    assert L.gsr_median_temp_bytes(100) == 800 and L.gsr_median_temp_bytes(0) == 0 and L.gsr_median_temp_bytes(-4) == 0
    assert re.search(r"#define\s+GSR_MEDIAN_NONE\s+0xFFFFFFFFu", text) and _capi.GSR_MEDIAN_NONE == 0xFFFFFFFF == NONE


def test_the_struct_is_the_headers_and_the_header_compiles_as_c(tmp_path):
    names = [n for n, _ in _capi.MedianArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_median_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_median_args, {f}));' for f in names)
    src, exe = tmp_path / "median_abi.c", tmp_path / "median_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_median.h"\nint main(void){' + body
                   + "int (*fn)(gsr_median_args*) = gsr_median_forward; (void)fn; fn = gsr_median_backward; (void)fn; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "median_abi.o")])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_median.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.MedianArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.MedianArgs, f).offset, f


# ---- 5. the error contract, without a device ------------------------------------------------------------------------------------
N, W, H, RENDERED = 100, 40, 24, 500
GEO, IMG, BIN, SCENE = 0x10000000, 0x20000000, 0x30000000, 0x40000000      # addresses nothing dereferences: every case is decided before


def valid_args(keep):
    """gsr_median_args that pass every check of both calls (they would launch). keep: receives the outputs and the scratch
    (ctypes holds addresses only), with a pattern no refused call may touch."""
    L = _capi.lib()
    bst = _capi.BinningState()
    L.gsr_binning_from_chunk(BIN, RENDERED, C.byref(bst))
    a = _capi.MedianArgs()
    a.struct_size = C.sizeof(_capi.MedianArgs)
    a.num_gaussians, a.width, a.height, a.threshold = N, W, H, 0.5
    a.means2D, a.conic_opacity = GEO + 0x1000, GEO + 0x2000
    a.ranges, a.n_contrib, a.final_t = IMG, IMG + 0x1000, IMG + 0x3000
    a.point_list = bst.values
    a.values, a.dL_dout = SCENE, SCENE + 0x20000
    r = a.receipt
    r.magic, r.plan_used = _capi.GSR_RECEIPT_MAGIC, 1
    r.num_gaussians, r.width, r.height, r.tile_row_begin, r.tile_row_end = N, W, H, 0, 2
    r.num_rendered, r.num_visible, r.serial = RENDERED, N, 0
    r.geometry_chunk, r.image_chunk, r.binning_chunk = GEO, IMG, BIN
    out, grad = (C.c_float * (W * H))(*([7.0] * (W * H))), (C.c_float * N)(*([7.0] * N))
    ids, dom = (C.c_uint32 * (W * H))(*([7] * (W * H))), (C.c_uint32 * (W * H))(*([7] * (W * H)))
    sums = (C.c_double * (N + 1))()
    keep.extend([out, grad, ids, dom, sums])
    a.out, a.dL_dvalues, a.ids, a.dominant_ids, a.value_sums_f64 = (C.addressof(v) for v in (out, grad, ids, dom, sums))
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


def _all(*changes):
    def change(a):
        for c in changes:
            c(a)
    return change


BOTH, FORWARD, BACKWARD = ("gsr_median_forward", "gsr_median_backward"), ("gsr_median_forward",), ("gsr_median_backward",)
REFUSALS = {
    "struct_size too small": (BOTH, _set("struct_size", C.sizeof(_capi.MedianArgs) - 8)),
    "struct_size too large": (BOTH, _set("struct_size", C.sizeof(_capi.MedianArgs) + 8)),
    "struct_size zero": (BOTH, _set("struct_size", 0)),
    "no Gaussians": (BOTH, _set("num_gaussians", 0)),
    "no width": (BOTH, _set("width", 0)),
    "a negative height": (BOTH, _set("height", -16)),
    "rows outside the frame": (BOTH, _set("tile_row_end", 3)),
    "rows the wrong way round": (BOTH, _all(_set("tile_row_begin", 2), _set("tile_row_end", 1))),
    "threshold 1": (FORWARD, _set("threshold", 1.0)),
    "threshold above 1": (FORWARD, _set("threshold", 1.5)),
    "a negative threshold": (FORWARD, _set("threshold", -1e-6)),
    "threshold NaN": (FORWARD, _set("threshold", float("nan"))),
    "threshold infinite": (FORWARD, _set("threshold", float("inf"))),
    "no receipt": (FORWARD, _set("receipt.magic", 0)),
    "a receipt of something else": (FORWARD, _set("receipt.magic", 0x12345678)),
    "another N": (FORWARD, _set("num_gaussians", N + 1)),
    "another width": (FORWARD, _set("width", W + 16)),
    "another height": (FORWARD, _set("height", H + 16)),
    "the receipt's N": (FORWARD, _set("receipt.num_gaussians", N - 1)),
    "rows the receipt does not have": (FORWARD, _set("receipt.tile_row_end", 1)),
    "a receipt whose rows leave the frame": (FORWARD, _set("receipt.tile_row_end", 3)),
    "point_list of another chunk": (FORWARD, _set("point_list", BIN + 0x40)),
    "no point_list": (FORWARD, _set("point_list", None)),
    "no binning chunk": (FORWARD, _set("receipt.binning_chunk", None)),
    "sorted lists skipped": (FORWARD, _set("receipt.plan_used", 2 | _capi.GSR_PLAN_LISTS_SKIPPED)),
    "no means2D": (FORWARD, _set("means2D", None)),
    "no conic_opacity": (FORWARD, _set("conic_opacity", None)),
    "no ranges": (FORWARD, _set("ranges", None)),
    "no n_contrib": (FORWARD, _set("n_contrib", None)),
    "no final_t": (FORWARD, _set("final_t", None)),
    "means2D off an 8-byte boundary": (FORWARD, _odd("means2D")),
    "ranges off an 8-byte boundary": (FORWARD, _odd("ranges")),
    "conic_opacity off a 16-byte boundary": (FORWARD, _odd("conic_opacity", 8)),
    "no output at all": (FORWARD, _all(_set("out", None), _set("ids", None), _set("dominant_ids", None))),
    "out without values": (FORWARD, _set("values", None)),
    "no ids": (BACKWARD, _set("ids", None)),
    "no dL_dout": (BACKWARD, _set("dL_dout", None)),
    "no dL_dvalues": (BACKWARD, _set("dL_dvalues", None)),
    "no scratch": (BACKWARD, _set("value_sums_f64", None)),
    "scratch off an 8-byte boundary": (BACKWARD, _odd("value_sums_f64")),
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
        assert all(set(v) == {7.0} for v in keep[:2]) and all(set(v) == {7} for v in keep[2:4]) and not any(keep[4])


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_decided_without_a_device(case):
    refused_untouched(case)


def test_null_args_are_refused():
    L = _capi.lib()
    for name in BOTH:
        assert getattr(L, name)(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
