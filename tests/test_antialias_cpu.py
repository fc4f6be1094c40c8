"""CPU: the opacity compensation (gsr_antialias_forward / _backward, include/gsrast_amd_antialias.h). The two references of
tests/antialias_ref.py against each other, the differentiable one against finite differences, what float32 alone does to
its gradients (the table BOUNDS), the leave-out rule and the blindness guards of the scenes tests/test_gpu_antialias.py
uses; the sixth header against its ctypes table; every refusal of the two calls without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import antialias_ref as R
from helpers import ROOT

from gsrast_amd import _capi

PROFILES = ("gscuda", "inria")
BOUND_SCENES = [(p, "conditioned") for p in PROFILES] + [(p, "composition") for p in PROFILES]


def _kept(semantics, which="conditioned"):
    scene, cam = R.conditioned_scene(semantics), R.camera(semantics)
    if which == "composition":
        scene, cam = R.composition_scene(semantics), R.composition_camera()
    near, agree = R.near_a_threshold(scene, cam, semantics)
    return scene, cam, R.masks_of(scene, cam, semantics), near, agree


# ---- the references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", PROFILES)
def test_float32_restatement_is_the_float64_function_to_rounding(semantics):
    """c <= 1 and c = sqrt(d0 / d1): the only amplifier of a rounding is the cancellation in d0 = a0 c0 - b b, by
    a0 c0 / d0, which the scene's per-axis spread of 0.3 keeps below ~30 for all but a few rows; a dozen roundings of 2^-24
    each lead to it: 30 x 12 x 2^-24 / 2 ~ 1e-5 of the largest entry (1)."""
    scene, cam, masks, near, agree = _kept(semantics)
    g = np.ones(len(near), np.float32)
    _, c64 = R.gradients(scene, cam, g, semantics, masks=masks)
    on = ~near
    err = float(np.abs(masks["c"].astype(np.float64) - c64)[on].max())
    print(f"{semantics}: max |c32 - c64| = {err:.2e}")
    assert err <= 1e-5
    # rows without a covariance: 1 exactly, o' = o bit for bit
    dead = masks["culled"] | masks["d1_bad"]
    assert (masks["c"][dead] == 1.0).all() and np.array_equal(masks["o_out"][dead].view(np.uint32), scene["opacities"][dead].view(np.uint32))
    assert np.array_equal(masks["o_out"], scene["opacities"] * masks["c"])


@pytest.mark.parametrize("semantics", PROFILES)
def test_differentiable_reference_against_finite_differences(semantics):
    scene, cam, masks, near, _ = _kept(semantics)
    rows = np.nonzero(masks["flows"] & ~near)[0][:300]
    sub = {k: v[rows] for k, v in scene.items()}
    sub_masks = {k: v[rows] for k, v in masks.items()}
    g = R.seed_gradient(len(rows), seed=9)
    grads, _ = R.gradients(sub, cam, g, semantics, masks=sub_masks)

    def loss_rows(s):
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)
        with torch.no_grad():
            out, _ = R.compensated(t(s["means3D"][:, :3]), t(s["scales"][:, :3]), t(s["rotations"]), t(s["opacities"]), cam.view,
                                   sub_masks, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, semantics)
        return out.numpy() * g.astype(np.float64)               # rows are independent: one difference per row at once
    base = {k: v.astype(np.float64) for k, v in sub.items()}
    at = np.abs(loss_rows(base))
    for name, key, comps in (("means3D", "means3D", 3), ("scales", "scales", 3), ("rotations", "rotations", 4)):
        for k in range(comps):
            h = 1e-6 * np.maximum(np.abs(base[key][:, k]), 1.0 if key == "means3D" else 1e-3)
            up, dn = {a: b.copy() for a, b in base.items()}, {a: b.copy() for a, b in base.items()}
            up[key][:, k] += h
            dn[key][:, k] -= h
            fd = (loss_rows(up) - loss_rows(dn)) / (2.0 * h)
            ref = grads[name][:, k]
            scale = np.maximum(np.abs(grads[name]).max(1), 1e-12)
            # (1e-5 of the row's gradient for the truncation, and the difference's own rounding: ~50 ulp of the loss over h)
            assert (np.abs(fd - ref) <= 1e-5 * scale + 1e-14 * at / h).all(), (name, k, float((np.abs(fd - ref) / scale).max()))
    assert np.allclose(grads["opacities"], g.astype(np.float64) * sub_masks["c"].astype(np.float64), rtol=1e-5)


@pytest.mark.parametrize("semantics,which", BOUND_SCENES)
def test_float32_error_of_the_gradients_and_the_bounds_table(semantics, which):
    scene, cam, masks, near, _ = _kept(semantics, which)
    g = R.seed_gradient(len(near))
    g64, _ = R.gradients(scene, cam, g, semantics, masks=masks)
    g32, _ = R.gradients(scene, cam, g, semantics, dtype=torch.float32, masks=masks)
    on = ~near
    for name in R.ARRAYS:
        top = float(np.abs(g64[name][on]).max())
        e32 = float(np.abs(g32[name][on] - g64[name][on]).max()) / top
        print(f"{semantics} {which} {name}: e32 = {e32:.2e} of the largest entry {top:.3e}")
        assert top > 0 and e32 <= 1e-3, "the scene is too anisotropic for a float64 comparison: make it rounder"
        want, key = max(R.FLOOR, 2.0 * e32), (semantics, which)
        if want > R.FLOOR:
            assert abs(R.bound(key, name) - want) <= 0.25 * want, (key, name, want)
        else:
            assert (key, name) not in R.BOUNDS and R.bound(key, name) == R.FLOOR


@pytest.mark.parametrize("semantics", PROFILES)
def test_composition_frame_holds_every_case(semantics):
    scene, cam, masks, near, agree = _kept(semantics, "composition")
    n = len(near)
    assert near.sum() <= R.MAX_LEFT_OUT * n and agree[~near].all()
    share = float((masks["c"][masks["flows"]] < 0.9).mean())
    print(f"{semantics}: {share:.2f} of the frame's live Gaussians have c < 0.9; {int(masks['culled'].sum())} culled")
    assert 0.35 <= share <= 0.75 and masks["culled"].sum() >= 10 and (masks["c"][masks["flows"]] > 0.95).sum() >= 10


def test_needles_are_beyond_float32():
    """Why the needle scene is compared float32 with float32 only: on it float32 loses c itself."""
    scene, cam = R.needle_scene("inria"), R.camera("inria")
    masks = R.masks_of(scene, cam, "inria")
    with np.errstate(all="ignore"):
        _, c64 = R.gradients(scene, cam, np.ones(1000, np.float32), "inria", masks=masks)
    on = masks["flows"] & np.isfinite(c64)
    assert float(np.abs(masks["c"].astype(np.float64) - c64)[on].max()) > 1e-3
    assert masks["d1_bad"].sum() >= 5 and masks["floored"].sum() >= 20 and np.isfinite(masks["c"]).all()


# ---- the leave-out rule and the blindness guards ------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", PROFILES)
def test_conditioned_scenes_hold_every_case(semantics):
    scene, cam, masks, near, agree = _kept(semantics)
    n = len(near)
    print(f"{semantics}: {int(near.sum())} of {n} rows left out")
    assert near.sum() <= R.MAX_LEFT_OUT * n
    assert agree[~near].all(), "a float32 decision differs from the float64 one away from its threshold"
    flows = masks["flows"] & ~near
    assert (masks["c"][flows] < 0.9).sum() >= 0.1 * n
    assert (masks["floored"] & ~near).sum() >= 20
    for k in ("hi_x", "lo_x", "hi_y", "lo_y"):
        assert (masks[k] & flows).sum() >= 20, k                # clamped rows that are not culled, on each side
    assert (masks["culled"] & ~near).sum() >= 20
    assert (flows & (masks["c"] > 0.99)).sum() >= 20            # and large splats the compensation leaves almost alone
    if semantics == "gscuda":
        norm = np.linalg.norm(scene["rotations"].astype(np.float64), axis=1)
        assert (np.abs(norm - 1.0) > 0.2).sum() >= 0.3 * n


def test_reference_profile_gradient_is_orthogonal_to_the_quaternion():
    """(its preprocess normalises q: c does not change along q, and a reference that skipped the normalisation would)"""
    scene, cam, masks, near, _ = _kept("gscuda")
    g64, _ = R.gradients(scene, cam, R.seed_gradient(len(near)), "gscuda", masks=masks)
    dot = (g64["rotations"] * scene["rotations"].astype(np.float64)).sum(1)
    assert np.abs(dot).max() <= 1e-9 * np.abs(g64["rotations"]).max() and np.abs(g64["rotations"]).max() > 0


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
HEADER = "gsrast_amd_antialias.h"
STRUCTS = {"gsr_antialias_args": _capi.AntialiasArgs, "gsr_antialias_backward_args": _capi.AntialiasBackwardArgs}


def _declared_functions():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_antialias_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_antialias_backward", "gsr_antialias_forward"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in {HEADER} but not exported"
    assert set(_capi.ANTIALIAS_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES):
        assert not set(_capi.ANTIALIAS_SIGNATURES) & set(other)


def test_the_structs_are_the_headers_and_the_header_compiles_as_c(tmp_path):
    body = ""
    for cname, cls in STRUCTS.items():
        body += f'printf("{cname} size %zu\\n", sizeof({cname}));'
        body += "".join(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    head = f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{'
    src, exe = tmp_path / "antialias_abi.c", tmp_path / "antialias_abi"
    src.write_text(head + body + "int (*f)(gsr_antialias_args*) = gsr_antialias_forward; (void)f;"
                   "int (*b)(gsr_antialias_backward_args*) = gsr_antialias_backward; (void)b; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "antialias_abi.o")])
    src.write_text(head + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls in STRUCTS.items():
        assert got[(cname, "size")] == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)


# ---- the error contract, without a device ----------------------------------------------------------------------------------------
N = 100
BASE = 0x10000000                 # addresses nothing dereferences: every case is decided before any HIP call


def _valid(backward, inria=False):
    a = (_capi.AntialiasBackwardArgs if backward else _capi.AntialiasArgs)()
    a.struct_size = C.sizeof(type(a))
    a.flags = _capi.GSR_FLAG_SEMANTICS_INRIA if inria else 0
    a.num_gaussians, a.width, a.height = N, 64, 48
    a.tan_fovx, a.tan_fovy, a.scale_modifier = 0.5, 0.4, 1.0
    a.means3D, a.scales, a.rotations, a.opacities = BASE, BASE + 0x1000, BASE + 0x2000, BASE + 0x3000
    a.view_matrix, a.proj_matrix = BASE + 0x4000, BASE + 0x4100
    if backward:
        a.dL_dopacities_out, a.radii = BASE + 0x5000, BASE + 0x6000
        a.dL_dopacities, a.dL_dmeans3D, a.dL_dscales, a.dL_drotations = BASE + 0x7000, BASE + 0x8000, BASE + 0x9000, BASE + 0xA000
    else:
        a.opacities_out, a.compensation = BASE + 0x5000, BASE + 0x6000
    return a


def _set(name, value):
    return lambda a: setattr(a, name, value)


def _no_outputs(a):
    if isinstance(a, _capi.AntialiasBackwardArgs):
        a.dL_dopacities = a.dL_dmeans3D = a.dL_dscales = a.dL_drotations = None
    else:
        a.opacities_out = a.compensation = None


COMMON_REFUSALS = {
    "struct_size too small": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) - 8),
    "struct_size too large": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) + 8),
    "struct_size zero": _set("struct_size", 0),
    "negative N": _set("num_gaussians", -1),
    "width zero": _set("width", 0),
    "height negative": _set("height", -4),
    "tan_fovx zero": _set("tan_fovx", 0.0),
    "tan_fovx NaN": _set("tan_fovx", float("nan")),
    "tan_fovy negative": _set("tan_fovy", -0.4),
    "tan_fovy infinite": _set("tan_fovy", float("inf")),
    "scale_modifier zero": _set("scale_modifier", 0.0),
    "scale_modifier NaN": _set("scale_modifier", float("nan")),
    "scale_modifier infinite": _set("scale_modifier", float("inf")),
    "no means3D": _set("means3D", None),
    "no scales": _set("scales", None),
    "no rotations": _set("rotations", None),
    "no opacities": _set("opacities", None),
    "no view_matrix": _set("view_matrix", None),
    "no proj_matrix under the reference profile": _set("proj_matrix", None),
    "an unknown flag": _set("flags", _capi.GSR_FLAG_PROFILE),
    "an unknown flag beside the profile's": _set("flags", _capi.GSR_FLAG_SEMANTICS_INRIA | 0x80000000),
    "means3D off a 16-byte boundary": _set("means3D", BASE + 4),
    "all outputs NULL": _no_outputs,
}
FORWARD_REFUSALS = dict(COMMON_REFUSALS)
FORWARD_REFUSALS["opacities_out aliases opacities"] = _set("opacities_out", BASE + 0x3000)
BACKWARD_REFUSALS = dict(COMMON_REFUSALS)
BACKWARD_REFUSALS["no dL_dopacities_out"] = _set("dL_dopacities_out", None)
BACKWARD_REFUSALS["dL_dscales off a 16-byte boundary"] = _set("dL_dscales", BASE + 0x9008)


def _refused(fn, a):
    L = _capi.lib()
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert fn(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""


@pytest.mark.parametrize("case", list(FORWARD_REFUSALS))
def test_every_forward_refusal_is_decided_without_a_device(case):
    a = _valid(False)
    FORWARD_REFUSALS[case](a)
    _refused(_capi.lib().gsr_antialias_forward, a)
    # ... and with N == 0 it stays a refusal
    a.num_gaussians = 0 if case != "negative N" else -1
    _refused(_capi.lib().gsr_antialias_forward, a)


@pytest.mark.parametrize("case", list(BACKWARD_REFUSALS))
def test_every_backward_refusal_is_decided_without_a_device(case):
    a = _valid(True)
    BACKWARD_REFUSALS[case](a)
    _refused(_capi.lib().gsr_antialias_backward, a)
    a.num_gaussians = 0 if case != "negative N" else -1
    _refused(_capi.lib().gsr_antialias_backward, a)


def test_null_args_and_an_empty_scene():
    L = _capi.lib()
    for fn in (L.gsr_antialias_forward, L.gsr_antialias_backward):
        assert fn(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    # N == 0: GSR_OK, nothing launched or written — no device needed; the upstream profile needs no proj_matrix; one output is enough
    for backward, fn in ((False, L.gsr_antialias_forward), (True, L.gsr_antialias_backward)):
        a = _valid(backward, inria=True)
        a.num_gaussians, a.proj_matrix = 0, None
        if backward:
            a.dL_dmeans3D = a.dL_dscales = a.dL_drotations = a.radii = None
        else:
            a.opacities_out = None
        assert fn(C.byref(a)) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
