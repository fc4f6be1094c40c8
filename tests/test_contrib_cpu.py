"""CPU: the per-Gaussian contribution statistics (gsr_contribution, include/gsrast_amd_contrib.h). The reference of
tests/contrib_ref.py by hand, against cpu_oracle.forward (its finalT / nContrib bit for bit on every scene
tests/test_gpu_contrib.py uses: what the GPU comparison rests on), against a float64 replay and against the forward's own
outputs; the scenes' blindness guards; the fifth header against its ctypes table; every refusal of the call without a device."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import contrib_ref as R
from helpers import ROOT
from oracle import cpu_oracle

from gsrast_amd import _capi

SCENES = {name: (scene, cam) for name, scene, cam in R.all_scenes()}
BOTH_SEMANTICS = ("edge", "fill", "views-0", "views-1")


@functools.lru_cache(maxsize=None)
def host(name, semantics="gscuda"):
    """(state of cpu_oracle.forward, reference over it) — under "inria" the same lists with the cut-off at 1e-4."""
    scene, cam = SCENES[name]
    state = host(name)[0] if semantics == "inria" else cpu_oracle.forward(scene, cam)
    return state, R.of_state(state, cam, semantics, wide=True)


# ---- the reference by hand ------------------------------------------------------------------------------------------------
def _stack(opacities, w=1, h=1, at=(0.0, 0.0)):
    """Round Gaussians centred on pixel `at`, front to back in the order given: there power = 0 and alpha = min(0.99, opacity)."""
    n = len(opacities)
    means = np.tile(np.asarray(at, np.float32), (n, 1))
    co = np.stack([np.full(n, 0.5), np.zeros(n), np.full(n, 0.5), np.asarray(opacities)], 1).astype(np.float32)
    return R.contribution(means, co, np.array([[0, n]], np.uint32), np.arange(n, dtype=np.uint32), w, h)


def test_one_gaussian_over_one_pixel():
    got = _stack([0.5])
    assert got["weight_sum"].tolist() == [1 << 31] and got["weight_max"].tolist() == [1 << 31]
    assert got["pixels"].tolist() == [1] and got["dominant"].tolist() == [1]
    assert got["finalT"][0, 0] == np.float32(0.5) and got["nContrib"][0, 0] == 1
    # alpha is capped at 0.99: q = trunc(0.99f * 2^32)
    assert _stack([1.0])["weight_max"].tolist() == [int(np.float32(0.99).astype(np.float64) * 2.0 ** 32)]
    # below 1/255: blended by nobody, dominant for nobody
    none = _stack([0.003])
    assert not any(none[k].any() for k in R.NAMES) and none["nContrib"][0, 0] == 0 and none["finalT"][0, 0] == 1.0


def test_two_stacked_and_the_record_a_pixel_stops_on():
    got = _stack([0.5, 0.5])
    assert got["weight_sum"].tolist() == [1 << 31, 1 << 30] and got["weight_max"].tolist() == [1 << 31, 1 << 30]
    assert got["pixels"].tolist() == [1, 1] and got["dominant"].tolist() == [1, 0]
    # over a 2 x 1 image the second pixel sees the same stack one pixel off centre: exp(-0.25) of the opacity
    wide = _stack([0.5, 0.5], w=2)
    off = np.float32(0.5) * cpu_oracle.expf(np.array([-0.25], np.float32))[0]
    q0 = int(np.float64(off) * 2.0 ** 32)
    q1 = int(np.float64(np.float32(off * (np.float32(1.0) - off))) * 2.0 ** 32)
    assert wide["weight_sum"].tolist() == [(1 << 31) + q0, (1 << 30) + q1] and wide["weight_max"].tolist() == [1 << 31, 1 << 30]
    assert wide["pixels"].tolist() == [2, 2] and wide["dominant"].tolist() == [2, 0]
    # 0.5, then two at 0.99: T = 1, 0.5, 0.005 — the third would leave 5e-5 < 0.001: the pixel stops ON it, and it is not blended
    stop = _stack([0.5, 1.0, 1.0])
    assert stop["pixels"].tolist() == [1, 1, 0] and stop["nContrib"][0, 0] == 2 and stop["stopped"][0, 0]
    assert stop["weight_sum"][2] == 0 and stop["weight_max"][2] == 0 and stop["dominant"].tolist() == [1, 0, 0]


def test_a_tie_for_dominant_goes_to_the_front_most():
    # alpha 0.2 then 0.25: w = 0.2f, and 0.25f * (1 - 0.2f) rounds to 0.2f again — the same q
    got = _stack([0.2, 0.25, 0.1])
    assert got["weight_max"][0] == got["weight_max"][1] > got["weight_max"][2] > 0
    assert got["dominant"].tolist() == [1, 0, 0] and got["pixels"].tolist() == [1, 1, 1]
    # ... and a later record wins only by being strictly larger
    assert _stack([0.2, 0.3])["dominant"].tolist() == [0, 1]


# ---- against the oracle, a float64 replay and the forward's own outputs -------------------------------------------------------
@pytest.mark.parametrize("name", list(SCENES))
def test_reference_forward_is_the_oracles_bit_for_bit(name):
    """The allowed mismatch is 0: the GPU's finalT / nContrib are the oracle's bit for bit (tests/test_gpu_parity.py), so the
    replay's alpha, T and decisions are the GPU's."""
    state, ref = host(name)
    assert np.array_equal(ref["finalT"].view(np.uint32), state["finalT"].view(np.uint32))
    assert np.array_equal(ref["nContrib"], state["nContrib"])
    if name in BOTH_SEMANTICS:
        cam = SCENES[name][1]
        exp = cpu_oracle.blend_cutoff(state, cam, t_cutoff=1e-4)
        ref4 = host(name, "inria")[1]
        assert np.array_equal(ref4["finalT"].view(np.uint32), exp["finalT"].view(np.uint32))
        assert np.array_equal(ref4["nContrib"], exp["nContrib"])


def identity_bound(ref, w, h):
    """2^-21 (sum_i pixels[i] + W H): each blended record contributes at most about three float32 roundings of magnitude
    <= 2^-24 T to its pixel's telescoping sum 1 - finalT = sum alpha_k T_k, plus 2^-32 of truncation."""
    return 2.0 ** -21 * (float(ref["pixels"].sum()) + w * h)


@pytest.mark.parametrize("name,semantics", [(n, "gscuda") for n in SCENES] + [(n, "inria") for n in BOTH_SEMANTICS])
def test_reference_identities_and_the_float64_replay(name, semantics):
    cam = SCENES[name][1]
    state, ref = host(name, semantics)
    # every pixel that blended something has exactly one dominant Gaussian
    assert int(ref["dominant"].sum()) == int((ref["nContrib"] > 0).sum())
    assert (ref["dominant"] <= ref["pixels"]).all() and ((ref["pixels"] > 0) == (ref["weight_max"] > 0)).all()
    assert (ref["weight_sum"] >= ref["weight_max"]).all() and (ref["weight_sum"] <= ref["pixels"] * ref["weight_max"].astype(np.uint64)).all()
    total = float(ref["weight_sum"].astype(np.float64).sum() * 2.0 ** -32)
    opacity = float((1.0 - ref["finalT"].astype(np.float64)).sum())
    bound = identity_bound(ref, cam.width, cam.height)
    print(f"{name} {semantics}: |sum weight - sum (1 - finalT)| = {abs(total - opacity):.3e}, {abs(total - opacity) / bound:.3f} of the bound")
    assert abs(total - opacity) <= bound
    # the float64 replay (same decisions): the frame's total under the same bound — a pixel's K blended records carry at most
    # (3 + 2 K) 2^-24 between them (T's drift grows by two roundings a record, and sum w <= 1) against (K + 1) 2^-21 —, and
    # each Gaussian within pixels[i] (3 + 2 K_max) 2^-24
    wide = ref["weight_sum_f64"]
    fixed = ref["weight_sum"].astype(np.float64) * 2.0 ** -32
    assert abs(fixed.sum() - wide.sum()) <= bound
    k_max = float(ref["nContrib"].max())
    assert (np.abs(fixed - wide) <= ref["pixels"].astype(np.float64) * (3.0 + 2.0 * k_max) * 2.0 ** -24).all()
    assert wide.sum() > 0 or name.startswith("tile-1")


# ---- blindness guards -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["edge", "fill"])
def test_mixed_scenes_hold_every_case(name):
    for semantics in ("gscuda", "inria"):
        state, ref = host(name, semantics)
        assert ((state["radii"] > 0) & (ref["pixels"] == 0)).any()      # a Gaussian with tiles that nothing blends
        assert ref["stopped"].any()                                     # a pixel that stops on the cut-off
        assert (ref["nContrib"] == 0).any()                             # a pixel that blends nothing
        assert (ref["dominant"] > 0).sum() > 20
    if name == "fill":
        # Gaussian 0 is blended in every one of the 64 tiles: 64 waves add into its row
        scene, cam = SCENES[name]
        state = host(name)[0]
        assert (state["ranges"][:, 1] > state["ranges"][:, 0]).all()
        d2 = (np.arange(128)[None, :] - state["means2D"][0, 0]) ** 2 + (np.arange(128)[:, None] - state["means2D"][0, 1]) ** 2
        reach = (d2.reshape(8, 16, 8, 16).min(axis=(1, 3)) < 70.0 ** 2)
        assert reach.all() and int(host(name)[1]["pixels"][0]) > 64 * 100


@pytest.mark.parametrize("length", R.LIST_LENGTHS)
def test_one_tile_scenes_have_their_list_and_their_walks(length):
    for opaque in (False, True):
        state, ref = host(f"tile-{length}-{'opaque' if opaque else 'faint'}")
        assert int(state["ranges"][0, 1]) - int(state["ranges"][0, 0]) == length
        assert (state["radii"] == 0).sum() >= 2                          # rows nothing ever touches
        if not opaque:
            assert not ref["stopped"].any()                              # every pixel walks to the end of the list
            assert int(ref["nContrib"].max()) == length
        elif length >= 63:
            stops = ref["nContrib"][ref["stopped"]]
            assert len(np.unique(stops)) >= 4 and (~ref["stopped"]).any()     # pixels stop at different depths, some never
        assert ref["pixels"].sum() > 0


def test_no_pixel_of_the_two_views_reaches_the_cutoff():
    for name in ("views-0", "views-1"):
        for semantics in ("gscuda", "inria"):
            state, ref = host(name, semantics)
            assert not ref["stopped"].any() and float(ref["finalT"].min()) > 0.01
            never = (state["radii"] > 0) & (ref["pixels"] == 0)
            assert never.sum() > 10 and (ref["pixels"] > 0).sum() > 50


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def _declared_functions():
    text = open(os.path.join(ROOT, "include", "gsrast_amd_contrib.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_contrib_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_contribution"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_contrib.h but not exported"
    assert set(_capi.CONTRIB_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES):
        assert not set(_capi.CONTRIB_SIGNATURES) & set(other)


def test_the_struct_is_the_headers_and_the_header_compiles_as_c(tmp_path):
    names = [n for n, _ in _capi.ContributionArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_contribution_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_contribution_args, {f}));' for f in names)
    src, exe = tmp_path / "contrib_abi.c", tmp_path / "contrib_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_contrib.h"\nint main(void){' + body
                   + "int (*fn)(gsr_contribution_args*) = gsr_contribution; (void)fn; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "contrib_abi.o")])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_contrib.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.ContributionArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.ContributionArgs, f).offset, f


# ---- the error contract, without a device --------------------------------------------------------------------------------------
N, W, H, RENDERED = 100, 40, 24, 500
GEO, IMG, BIN = 0x10000000, 0x20000000, 0x30000000        # chunk addresses nothing dereferences: every case is decided before


def _valid_args(keep):
    """gsr_contribution_args that pass every check (the call would launch): a receipt as gsr_forward issues it. keep: the
    list the four output arrays are appended to (ctypes holds addresses only)."""
    L = _capi.lib()
    bst = _capi.BinningState()
    L.gsr_binning_from_chunk(BIN, RENDERED, C.byref(bst))
    a = _capi.ContributionArgs()
    a.struct_size = C.sizeof(_capi.ContributionArgs)
    a.num_gaussians, a.width, a.height = N, W, H
    a.means2D, a.conic_opacity, a.ranges, a.n_contrib = GEO + 0x1000, GEO + 0x2000, IMG, IMG + 0x1000
    a.point_list = bst.values
    r = a.receipt
    r.magic, r.plan_used = _capi.GSR_RECEIPT_MAGIC, 1
    r.num_gaussians, r.width, r.height, r.tile_row_begin, r.tile_row_end = N, W, H, 0, 2
    r.num_rendered, r.num_visible, r.serial = RENDERED, N, 1
    r.geometry_chunk, r.image_chunk, r.binning_chunk = GEO, IMG, BIN
    out = [(C.c_uint64 * N)(), (C.c_uint32 * N)(), (C.c_uint64 * N)(), (C.c_uint64 * N)()]
    keep.extend(out)
    a.weight_sum, a.weight_max, a.pixels, a.dominant = (C.addressof(o) for o in out)
    return a


def _set(path, value):
    def change(a):
        obj = a
        *head, last = path.split(".")
        for h in head:
            obj = getattr(obj, h)
        setattr(obj, last, value)
    return change


def _no_outputs(a):
    a.weight_sum = a.weight_max = a.pixels = a.dominant = None


REFUSALS = {
    "struct_size too small": _set("struct_size", C.sizeof(_capi.ContributionArgs) - 8),
    "struct_size too large": _set("struct_size", C.sizeof(_capi.ContributionArgs) + 8),
    "struct_size zero": _set("struct_size", 0),
    "no receipt": _set("receipt.magic", 0),
    "a receipt of something else": _set("receipt.magic", 0x12345678),
    "another N": _set("num_gaussians", N + 1),
    "another width": _set("width", W + 16),
    "another height": _set("height", H + 16),
    "the receipt's N": _set("receipt.num_gaussians", N - 1),
    "rows outside the frame": _set("receipt.tile_row_end", 3),
    "point_list of another chunk": _set("point_list", BIN + 0x40),
    "no point_list": _set("point_list", None),
    "no binning chunk": _set("receipt.binning_chunk", None),
    "sorted lists skipped": _set("receipt.plan_used", 2 | _capi.GSR_PLAN_LISTS_SKIPPED),
    "all four outputs NULL": _no_outputs,
    "no n_contrib": _set("n_contrib", None),
}


@pytest.mark.parametrize("case", list(REFUSALS))
def test_every_refusal_is_decided_without_a_device(case):
    L = _capi.lib()
    keep = []
    a = _valid_args(keep)
    REFUSALS[case](a)
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert L.gsr_contribution(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""
    assert not any(any(o) for o in keep)


def test_null_args_and_a_frame_that_rendered_nothing():
    L = _capi.lib()
    assert L.gsr_contribution(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    # R == 0: GSR_OK, nothing written, no binning chunk needed — and no device either
    keep = []
    a = _valid_args(keep)
    for w in keep:
        for i in range(N):
            w[i] = 7
    a.receipt.num_rendered, a.receipt.binning_chunk, a.point_list = 0, None, None
    a.stage_ms = 5.0
    assert L.gsr_contribution(C.byref(a)) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert all(list(o) == [7] * N for o in keep) and a.stage_ms == 0.0
    # ... but a refusal stays one whatever R is
    _no_outputs(a)
    assert L.gsr_contribution(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
