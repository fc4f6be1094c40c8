"""CPU: gsr_backward's argument contract and per-call constants (gsrast_amd/csrc/backward_policy.hpp). A small C++ driver is
compiled against the header with g++ (no HIP, no GPU). The table below is written from the comments of gsr_backward_args in
include/gsrast_amd.h: each legal argument set names, pointer by pointer, whether the call survives without it, and every
case breaks one rule only. The GPU tests show what a legal call computes; these show which calls are legal."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from helpers import ROOT

from gsrast_amd import _capi
from gsrast_amd.backward_plan import ROW_FLOATS

# every pointer of gsr_backward_args; the driver sets those of a case's bit mask to a dummy address (nothing is dereferenced)
POINTERS = ["background", "means2D", "conic_opacity", "colors", "cov3D", "radii", "ranges", "n_contrib", "final_t", "point_list",
            "means3D", "view_matrix", "dL_dout_color", "dL_dmean2D", "dL_dconic_opacity", "dL_dcolors", "dL_dcov3D", "dL_dshs",
            "dL_dcov2D", "sums_f64", "proj_matrix", "scales", "rotations", "dL_dmeans3D", "dL_dscales", "dL_drotations", "cam_pos",
            "shs", "clamped", "dL_dout_depth", "dL_ddepths", "depth_sums_f64"]

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "backward_policy.hpp"
using namespace gsr;
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
int main() {
    static char dummy[16];
    char what[16];
    while (std::scanf("%15s", what) == 1) {
        if (what[0] == 'c') {                     // choose: flags n width height row_begin row_end magic mask
            gsr_backward_args a;
            std::memset(&a, 0, sizeof(a));
            unsigned long long mask;
            std::scanf("%u %d %d %d %d %d %u %llu", &a.flags, &a.num_gaussians, &a.width, &a.height, &a.tile_row_begin,
                       &a.tile_row_end, &a.receipt.magic, &mask);
@SET_POINTERS@
            BackwardChoice c{};
            const int rc = choose_backward(a, &c);
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d\n", rc, c.wide, c.chain, c.depth, c.inria, c.have_receipt, c.profile,
                        c.depth_inverse, c.d.row_begin, c.d.row_end, c.d.grid_x, c.d.grid_y);
        } else if (what[0] == 'b') {              // band: width height row_begin row_end
            int w, h, b, e;
            std::scanf("%d %d %d %d", &w, &h, &b, &e);
            FrameDims d{};
            const int rc = tile_band(w, h, b, e, &d);
            std::printf("%d %d %d %d %d\n", rc, d.row_begin, d.row_end, d.grid_x, d.grid_y);
        } else if (what[0] == 'l') {              // lens: inria width height tan_fovx tan_fovy sh_dims
            int inria, w, h, sh; float tx, ty;
            std::scanf("%d %d %d %f %f %d", &inria, &w, &h, &tx, &ty, &sh);
            const ProfileLens l = profile_lens(inria != 0, w, h, tx, ty, sh);
            const float fy = (float)h / (2.0f * ty), fx = inria ? (float)w / (2.0f * tx) : (float)h / (2.0f * ty);
            const float eps = inria ? 0.0000001f : 0.001f;
            std::printf("%d %u %u %u %d\n", l.focal_x == fx && l.focal_y == fy && l.w_eps == eps, bits(l.focal_x), bits(l.focal_y),
                        bits(l.w_eps), l.sh_deg);
        } else {                                  // table: the number of sums arrays, then (offset, floats per row) per entry
            gsr_backward_args a;
            std::printf("%d", kBackwardSums);
            for (const BackwardOutput& o : kBackwardOutputs)
                std::printf(" %zu %d", (size_t)((const char*)&(a.*o.array) - (const char*)&a), o.row_floats);
            std::printf("\n");
        }
    }
    return 0;
}
""".replace("@SET_POINTERS@", "\n".join(
    f"            if (mask >> {i} & 1) a.{name} = reinterpret_cast<decltype(a.{name})>(dummy);" for i, name in enumerate(POINTERS)))

INRIA, PROFILE, DEPTH_INVERSE = _capi.GSR_FLAG_SEMANTICS_INRIA, _capi.GSR_FLAG_PROFILE, _capi.GSR_FLAG_DEPTH_INVERSE
OK, INVALID = _capi.GSR_OK, _capi.GSR_ERR_INVALID_ARG
REQ, OPT = True, False

# "state of the forward call" and dL_dout_color; point_list because these calls carry no receipt
ALWAYS = {k: REQ for k in ("background", "means2D", "conic_opacity", "colors", "ranges", "n_contrib", "final_t", "dL_dout_color",
                           "point_list")}
SUMS = ("dL_dmean2D", "dL_dconic_opacity", "dL_dcolors")
CHAIN_STATE = {k: REQ for k in ("cov3D", "means3D", "view_matrix", "radii")}
# (name: flags, {pointer: whether the call needs it WHILE THE OTHERS ARE GIVEN}, the modes expected of the whole set)
LEGAL_SETS = {
    # without sums_f64 the three arrays of the sums are required; dL_dcov2D is optional everywhere
    "narrow_sums": (0, {**ALWAYS, **{k: REQ for k in SUMS}, "dL_dcov2D": OPT}, dict(wide=0, chain=0, depth=0)),
    # ... and dL_dmeans3D / dL_dscales / dL_drotations need dL_dcov3D; dL_dmeans3D needs the projection, dL_drotations needs
    # dL_dscales, either needs the scales and rotations
    "narrow_chain": (0, {**ALWAYS, **{k: REQ for k in SUMS}, **CHAIN_STATE, "dL_dcov3D": REQ, "dL_dcov2D": OPT, "dL_dshs": OPT,
                         "dL_dmeans3D": OPT, "proj_matrix": REQ, "dL_dscales": REQ, "dL_drotations": OPT, "scales": REQ,
                         "rotations": REQ}, dict(wide=0, chain=1, depth=0)),
    # every output is optional once sums_f64 is given — which this set, complete for the narrow mode too, survives losing;
    # the depth channel needs means3D and the view, and depth_sums_f64 beside sums_f64 (dL_ddepths optional then)
    "wide_all_depth": (0, {**ALWAYS, **{k: OPT for k in SUMS}, **CHAIN_STATE, "sums_f64": OPT, "dL_dcov3D": OPT, "dL_dcov2D": OPT,
                           "dL_dshs": OPT, "dL_dmeans3D": OPT, "proj_matrix": REQ, "dL_dscales": REQ, "dL_drotations": OPT,
                           "scales": REQ, "rotations": REQ, "dL_dout_depth": OPT, "depth_sums_f64": REQ, "dL_ddepths": OPT},
                       dict(wide=1, chain=1, depth=1)),
    # the upstream profile's dL_dshs needs cam_pos, shs, clamped (and means3D, which the chain needs anyway); without
    # dL_dcov3D a narrow call runs no chain and is legal still
    "inria_shs": (INRIA, {**ALWAYS, **{k: REQ for k in SUMS}, **CHAIN_STATE, "dL_dcov3D": OPT, "dL_dshs": OPT, "shs": REQ,
                          "cam_pos": REQ, "clamped": REQ}, dict(wide=0, chain=1, depth=0, inria=1)),
}
REMOVALS = [(name, p) for name, (_, ptrs, _) in LEGAL_SETS.items() for p in ptrs]

CHOICE = ["rc", "wide", "chain", "depth", "inria", "have_receipt", "profile", "depth_inverse", "row_begin", "row_end", "grid_x",
          "grid_y"]
BAND = ["rc", "row_begin", "row_end", "grid_x", "grid_y"]
# 17 x 17 pixels: a grid of 2 x 2 tiles
BANDS = [((0, 0), dict(rc=OK, row_begin=0, row_end=2, grid_x=2, grid_y=2)),
         ((-1, 1), dict(rc=INVALID)), ((0, 3), dict(rc=INVALID)), ((2, 1), dict(rc=INVALID)),
         ((1, 1), dict(rc=OK, row_begin=1, row_end=1, grid_x=2, grid_y=2)),
         ((1, 2), dict(rc=OK, row_begin=1, row_end=2)), ((0, 2), dict(rc=OK, row_begin=0, row_end=2))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("backward_policy")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gsrast_amd", "csrc"),
                           str(d / "driver.cpp"), "-o", str(exe)])
    return str(exe)


def _run(driver, line):
    return subprocess.check_output([driver], input=line + "\n", text=True).split()


def _choose(driver, pointers, flags=0, n=8, width=17, height=17, rows=(0, 0), magic=0):
    mask = sum(1 << POINTERS.index(p) for p in pointers)
    out = _run(driver, f"choose {flags} {n} {width} {height} {rows[0]} {rows[1]} {magic} {mask}")
    return dict(zip(CHOICE, map(int, out)))


def test_header_needs_no_hip():
    text = open(os.path.join(ROOT, "gsrast_amd", "csrc", "backward_policy.hpp")).read()
    assert "hip_runtime" not in text and "gsr_common.hpp" not in text


def test_the_table_names_every_pointer_of_the_struct():
    fields = [n for n, t in _capi.BackwardArgs._fields_ if isinstance(t, type) and issubclass(t, (C._Pointer, C.c_void_p))]
    assert sorted(fields) == sorted(POINTERS + ["stream"])


@pytest.mark.parametrize("name", list(LEGAL_SETS))
def test_legal_set_and_its_modes(driver, name):
    flags, ptrs, modes = LEGAL_SETS[name]
    got = _choose(driver, ptrs, flags)
    assert got["rc"] == OK, got
    assert {k: got[k] for k in modes} == modes
    assert (got["have_receipt"], got["profile"], got["depth_inverse"]) == (0, 0, 0)
    assert (got["row_begin"], got["row_end"], got["grid_x"], got["grid_y"]) == (0, 2, 2, 2)


@pytest.mark.parametrize("name,pointer", REMOVALS, ids=[f"{n}-{p}" for n, p in REMOVALS])
def test_one_pointer_removed(driver, name, pointer):
    flags, ptrs, _ = LEGAL_SETS[name]
    got = _choose(driver, [p for p in ptrs if p != pointer], flags)
    assert got["rc"] == (INVALID if ptrs[pointer] else OK), (name, pointer, got)


def test_modes_follow_the_pointers_and_flags(driver):
    flags, ptrs, _ = LEGAL_SETS["wide_all_depth"]
    outputs = set(ROW_FLOATS) | {"dL_ddepths"}
    bare = [p for p in ptrs if p not in outputs]
    # with sums_f64 the chain runs for whichever of its outputs is asked for (dL_drotations alone is no legal request)
    assert _choose(driver, bare)["chain"] == 0
    for out in ("dL_dcov3D", "dL_dshs", "dL_dmeans3D", "dL_dscales"):
        got = _choose(driver, bare + [out])
        assert (got["rc"], got["wide"], got["chain"], got["depth"]) == (OK, 1, 1, 1), out
    assert _choose(driver, bare + ["dL_drotations"])["rc"] == INVALID
    # without it the chain starts from dL_dcov3D; dL_dshs alone asks for nothing
    narrow = [p for p in bare if p not in ("sums_f64", "dL_dout_depth", "depth_sums_f64")] + list(SUMS)
    assert _choose(driver, narrow + ["dL_dshs"])["chain"] == 0
    assert _choose(driver, narrow + ["dL_dmeans3D"])["rc"] == INVALID
    # the narrow depth channel keeps its sums in dL_ddepths
    assert _choose(driver, narrow + ["dL_dout_depth"])["rc"] == INVALID
    got = _choose(driver, narrow + ["dL_dout_depth", "dL_ddepths"])
    assert (got["rc"], got["wide"], got["depth"]) == (OK, 0, 1)
    got = _choose(driver, ptrs, INRIA | PROFILE | DEPTH_INVERSE)
    assert got["rc"] == INVALID                                       # (the upstream profile's dL_dshs: no shs)
    got = _choose(driver, [p for p in ptrs if p != "dL_dshs"], INRIA | PROFILE | DEPTH_INVERSE)
    assert (got["rc"], got["inria"], got["profile"], got["depth_inverse"]) == (OK, 1, 1, 1)


def test_sizes_and_the_receipt(driver):
    _, ptrs, _ = LEGAL_SETS["narrow_sums"]
    for bad in (dict(n=0), dict(n=-1), dict(width=0), dict(height=0), dict(height=-16)):
        assert _choose(driver, ptrs, **bad)["rc"] == INVALID, bad
    # with a receipt the lists are found through it: point_list may be missing (a magic that is not the library's is
    # refused later, where the receipt is read)
    no_list = [p for p in ptrs if p != "point_list"]
    got = _choose(driver, no_list, magic=_capi.GSR_RECEIPT_MAGIC)
    assert (got["rc"], got["have_receipt"]) == (OK, 1)
    assert _choose(driver, no_list, magic=5)["have_receipt"] == 1
    assert _choose(driver, no_list)["rc"] == INVALID


@pytest.mark.parametrize("rows,expected", BANDS, ids=[f"{b}_{e}" for (b, e), _ in BANDS])
def test_tile_band(driver, rows, expected):
    got = dict(zip(BAND, map(int, _run(driver, f"band 17 17 {rows[0]} {rows[1]}"))))
    assert {k: got[k] for k in expected} == expected
    # ... and gsr_backward's rules take the same band
    got = _choose(driver, LEGAL_SETS["narrow_sums"][1], rows=rows)
    assert {k: got[k] for k in expected} == expected


def test_tile_band_of_a_wide_image(driver):
    got = dict(zip(BAND, map(int, _run(driver, "band 1920 1080 60 68"))))
    assert got == dict(rc=OK, row_begin=60, row_end=68, grid_x=120, grid_y=68)
    assert int(_run(driver, "band 1920 1080 60 69")[0]) == INVALID


@pytest.mark.parametrize("inria", [0, 1])
def test_profile_lens(driver, inria):
    """gscuda: one focal length, H / (2 tan_fovy), and w + 0.001; upstream: two focal lengths and w + 1e-7."""
    w, h, tx, ty = 1237, 715, 0.7002075, 0.4142135
    f32 = np.float32
    fy = f32(h) / (f32(2.0) * f32(ty))
    fx = f32(w) / (f32(2.0) * f32(tx)) if inria else fy
    eps = f32(1e-7) if inria else f32(0.001)
    for sh_dims, deg in ((-1, 0), (0, 0), (3, 3), (9, 3), (2, 2)):
        same, bx, by, be, got_deg = map(int, _run(driver, f"lens {inria} {w} {h} {tx} {ty} {sh_dims}"))
        assert same == 1                          # the literal float expressions, compared with == in the driver
        assert (bx, by, be) == tuple(int(v.view(np.uint32)) for v in (fx, fy, eps))
        assert got_deg == deg
    assert fx != fy or not inria


def test_clearing_table(driver):
    """The table the two clearing loops walk: every per-Gaussian output array with its row width, the arrays the render
    backward's atomics add into first."""
    out = list(map(int, _run(driver, "table")))
    sums, pairs = out[0], list(zip(out[1::2], out[2::2]))
    name_at = {getattr(_capi.BackwardArgs, n).offset: n for n, _ in _capi.BackwardArgs._fields_}
    got = [(name_at[off], row) for off, row in pairs]
    expected = {**ROW_FLOATS, "dL_ddepths": 1}
    assert len(got) == len(expected) == 10 and dict(got) == expected
    assert {n for n, _ in got[:sums]} == {"dL_dmean2D", "dL_dconic_opacity", "dL_dcolors", "dL_dcov2D", "dL_ddepths"}
