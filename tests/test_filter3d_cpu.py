"""CPU: the 3D smoothing filter (gsr_filter3d_*, include/gsrast_amd_filter3d.h). The float32 restatements of
tests/filter3d_ref.py by hand and against the float64 transcription of upstream's compute_3D_filter, the float64 smoothing
against finite differences, what float32 alone does to the coefficient at extreme scales, camera_records against hand
values; the seventh header against its ctypes table; every refusal of the five calls without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import filter3d_ref as R
from helpers import ROOT

from gsrast_amd import _capi, filter3d

F = np.float32


# ---- the restatements by hand -----------------------------------------------------------------------------------------------
def test_observe_restatement_on_written_out_points():
    rec, max_focal = filter3d.camera_records([R.exact_camera()])
    assert max_focal == 512.0
    pts = np.array([[0.0, 0.0, 2.0],          # centre, depth 2: px = 320, py = 240
                    [-0.8125, 0.0, 1.0],      # px = -0.8125 * 512 + 320 = -96: on x_lo, valid
                    [1.0, 0.0, 1.0],          # px = 832 > 736: outside
                    [0.0, 0.0, 0.1],          # nearer than 0.2
                    [0.0, 0.0, -3.0]], F)     # behind
    md, detail = R.observe_f32(pts, rec, detail=True)
    d = detail[0]
    assert d["px"].tolist()[:3] == [320.0, -96.0, 832.0] and d["py"].tolist()[:3] == [240.0, 240.0, 240.0]
    assert d["valid"].tolist() == [True, True, False, False, False]
    assert md.tolist() == [2.0, 1.0, np.inf, np.inf, np.inf]
    # the clamp: behind the camera zc = 0.001, so px = (0 / 0.001) * 512 + 320
    assert d["px"][4] == 320.0 and not d["depth_ok"][4]
    # a second camera further away does not raise the minimum; a running minimum below is respected
    assert R.observe_f32(pts, rec, min_depth=np.array([0.5, 3.0, 7.0, np.inf, np.inf], F)).tolist() == [0.5, 1.0, 7.0, np.inf, np.inf]


def test_finalize_restatement_on_written_out_points():
    md = np.array([2.0, np.inf, 8.0, 0.5], F)
    got = R.finalize_f32(md, 512.0)
    want = [F(F(v) / F(512.0)) * R.K for v in (2.0, 8.0, 8.0, 0.5)]
    assert got.tolist() == [float(v) for v in want]
    assert R.K.view(np.uint32) == 0x3EE4F92E and R.K == F(0.2 ** 0.5) and float(R.K) == 0.4472135901451111
    none = R.finalize_f32(np.full(3, np.inf, F), 512.0)
    assert (none.view(np.uint32) == 0).all()


def test_forward_restatement_on_written_out_points():
    scales = np.array([[3.0, 4.0, 0.0, 2.5], [1.0, 1.0, 1.0, 7.0], [2.0, 2.0, 2.0, 1.0]], F)
    o = np.array([0.5, 0.25, 0.75], F)
    f = np.array([4.0, 0.0, 1e-30], F)                # 1e-30 squared underflows: IDENTITY, like 0
    got = R.forward_f32(scales, o, f)
    assert got["identity"].tolist() == [False, True, True]
    # row 0: s' = (5, sqrt(32), 4), r = (9/25, 16/32, 0): coef = 0
    assert got["scales_out"][0].tolist() == [5.0, float(np.sqrt(F(32.0))), 4.0, 2.5] and got["opacities_out"][0] == 0.0
    assert np.array_equal(got["scales_out"][1:].view(np.uint32), scales[1:].view(np.uint32))
    assert np.array_equal(got["opacities_out"][1:].view(np.uint32), o[1:].view(np.uint32))
    one = R.forward_f32(np.array([[3.0, 3.0, 3.0, 0.0]], F), np.array([1.0], F), np.array([4.0], F))
    r = F(9.0) / F(25.0)
    assert one["opacities_out"][0] == np.sqrt(F(F(r * r) * r)) and one["scales_out"][0, :3].tolist() == [5.0, 5.0, 5.0]


# ---- the restatement against upstream's loop ----------------------------------------------------------------------------------------
SCENE_N, SCENE_CAMERAS = 300, 5


def _seeded_scene():
    """The first seed whose scene passes the guard (chosen here, on the CPU; no row is excluded)."""
    for seed in range(50):
        pts, cams = R.seeded_points(SCENE_N, seed=seed, spread=6.0), R.orbit_cameras(SCENE_CAMERAS, seed=seed)
        if R.boundary_guard(pts, cams):
            return seed, pts, cams
    raise AssertionError("no seed passes the boundary guard")


def test_restatement_is_upstreams_loop_to_rounding():
    """Away from the five boundaries the float32 decisions are the float64 ones, so every row's depth is the same camera's
    t_2, which differs by the rounding of a four-term float32 sum: at most 8 x 2^-24 x (sum |terms of t_2|) / |t_2| relatively."""
    seed, pts, cams = _seeded_scene()
    print(f"seed {seed}")
    assert R.boundary_guard(pts, cams)
    rec, max_focal = filter3d.camera_records(cams)
    md = R.observe_f32(pts, rec)
    _, distance, valid_points, _ = R.upstream_filter64(pts, cams, detail=True)
    seen = md < np.inf
    assert np.array_equal(seen, valid_points) and 0.2 < seen.mean() < 1.0 and (~seen).sum() >= 10
    # per row: the largest sum |terms| / |t_2| over the cameras (the camera that gave the minimum is one of them)
    x = pts[:, :3].astype(np.float64)
    worst = np.zeros(len(pts))
    for c in rec.astype(np.float64):
        terms = np.abs(c[8] * x[:, 0]) + np.abs(c[9] * x[:, 1]) + np.abs(c[10] * x[:, 2]) + abs(c[11])
        t2 = c[8] * x[:, 0] + c[9] * x[:, 1] + c[10] * x[:, 2] + c[11]
        worst = np.maximum(worst, np.where(np.abs(t2) > 0.1, terms / np.maximum(np.abs(t2), 1e-300), 0.0))
    rel = np.abs(md[seen].astype(np.float64) - distance[seen]) / distance[seen]
    # (the view matrix itself is float32 in both: upstream_cameras reads the same Camera)
    assert (rel <= 8.0 * 2.0 ** -24 * worst[seen]).all(), float((rel / (2.0 ** -24 * worst[seen])).max())
    # and the filter: the same fill and factor (one more division, product and the rounding of K and f_x: 4 x 2^-24 more)
    got = R.finalize_f32(md, max_focal)
    want = R.upstream_filter64(pts, cams)
    bound = 8.0 * 2.0 ** -24 * np.where(seen, worst, worst[seen].max()) + 4.0 * 2.0 ** -24
    assert (np.abs(got - want) <= bound * want).all()
    assert (got[~seen] == got[seen].max()).all()


def test_batches_and_orders_agree_in_the_restatement():
    _, pts, cams = _seeded_scene()
    rec, _ = filter3d.camera_records(cams)
    whole = R.observe_f32(pts, rec)
    assert np.array_equal(R.observe_f32(pts, rec[3:], min_depth=R.observe_f32(pts, rec[:3])), whole)
    assert np.array_equal(R.observe_f32(pts, rec[::-1]), whole)


# ---- the float64 smoothing -------------------------------------------------------------------------------------------------------
def test_float64_smoothing_against_finite_differences():
    rng = np.random.default_rng(3)
    n = 200
    scales = np.exp(rng.uniform(-4.0, 1.0, (n, 4))) * np.where(rng.uniform(size=(n, 4)) < 0.2, -1.0, 1.0)
    o, f = rng.uniform(0.05, 0.95, n), np.exp(rng.uniform(-4.0, 1.0, n))
    f[:20] = 0.0
    gs, go = rng.normal(size=(n, 4)), rng.normal(size=n)
    identity = f == 0.0
    ref = R.gradients64(scales, o, f, gs, go, identity=identity)

    def loss(s, op):
        with torch.no_grad():
            sp, o2 = R.smoothing64(torch.from_numpy(s[:, :3].copy()), torch.from_numpy(op.copy()), torch.from_numpy(f), identity)
        return (sp.numpy() * gs[:, :3]).sum(1) + o2.numpy() * go          # rows are independent: one difference per row at once
    for j in range(3):
        h = 1e-6 * np.abs(scales[:, j])
        up, dn = scales.copy(), scales.copy()
        up[:, j] += h
        dn[:, j] -= h
        fd = (loss(up, o) - loss(dn, o)) / (2.0 * h)
        scale = np.maximum(np.abs(ref["scales"]).max(1), 1e-12)
        assert (np.abs(fd - ref["scales"][:, j]) <= 1e-6 * scale + 1e-9).all(), j
    h = 1e-6
    fd = (loss(scales, o + h) - loss(scales, o - h)) / (2.0 * h)
    assert np.allclose(fd, ref["opacities"], rtol=1e-7, atol=1e-9)
    assert np.array_equal(ref["scales"][identity], gs[identity, :3]) and np.array_equal(ref["opacities"][identity], go[identity])
    # the header's closed form is that function
    a = scales[:, :3] ** 2 + (f ** 2)[:, None]
    u = np.abs(scales[:, :3]) / np.sqrt(a)
    closed = gs[:, :3] * scales[:, :3] / np.sqrt(a)
    for j in range(3):
        closed[:, j] += o * go * np.sign(scales[:, j]) * f ** 2 / (a[:, j] * np.sqrt(a[:, j])) * u[:, (j + 1) % 3] * u[:, (j + 2) % 3]
    on = ~identity
    assert np.allclose(closed[on], ref["scales"][on], rtol=1e-12, atol=1e-300)
    assert np.allclose((u[:, 0] * u[:, 1] * u[:, 2] * go)[on], ref["opacities"][on], rtol=1e-12)


def test_ratio_product_survives_float32_where_the_determinants_do_not():
    values = np.array([1e-20, 1e-10, 1e-3, 1.0, 1e3, 1e9], F)
    grid = np.array([[a, b, c, 0.0] for a in values for b in values for c in values], F)
    for f in (1e-3, 1.0):
        filt = np.full(len(grid), f, F)
        got = R.forward_f32(grid, np.ones(len(grid), F), filt)
        assert np.isfinite(got["coef"]).all() and (got["coef"] >= 0).all() and (got["coef"] <= 1).all()
        assert np.isfinite(got["scales_out"]).all()
        # the blindness guard for that choice: upstream's form gives NaN on this grid (inf / inf at 1e9, 0 / 0 at 1e-20)
        assert np.isnan(R.det_ratio_coef_f32(grid, filt)).sum() >= 2
        # where upstream's form is well conditioned the two agree
        mid = ((grid[:, :3] >= 1e-3) & (grid[:, :3] <= 1e3)).all(1)
        assert np.allclose(got["coef"][mid], R.det_ratio_coef_f32(grid, filt)[mid], rtol=1e-5)


# ---- camera_records --------------------------------------------------------------------------------------------------------------
def test_camera_records_against_hand_values():
    from gsrast_amd.camera import first_person_camera
    cam = first_person_camera((1.0, 2.0, -5.0), 0.3, -0.1, 0.8, 0.05, 50.0, 100, 60)
    rec, max_focal = filter3d.camera_records([cam, R.exact_camera()])
    assert rec.shape == (2, 20) and rec.dtype == np.float32
    V = cam.view.reshape(4, 4).T
    assert np.array_equal(rec[0, :12], V[:3, :].reshape(12)) and V[2, 3] > 0      # row 2 points forward: the origin is in front
    assert rec[0, 12] == F(100.0) / (F(2.0) * F(cam.tan_fovx)) and rec[0, 13] == F(60.0) / (F(2.0) * F(cam.tan_fovy))
    assert rec[0, 14:].tolist() == [50.0, 30.0, float(F(-15.0)), float(F(100 * 1.15)), float(F(-0.15 * 60)), float(F(1.15 * 60))]
    assert rec[1, 12:].tolist() == [512.0, 512.0, 320.0, 240.0, -96.0, 736.0, -72.0, 552.0]
    assert max_focal == float(max(rec[0, 12], rec[1, 12]))
    # the tuple form, a tensor view included
    tup = (torch.from_numpy(cam.view.copy()), cam.tan_fovx, cam.tan_fovy, 100, 60)
    assert np.array_equal(filter3d.camera_records([tup])[0][0], rec[0])
    with pytest.raises(ValueError):
        filter3d.camera_records([(cam.view[:12], 0.5, 0.5, 10, 10)])
    empty, mf = filter3d.camera_records([])
    assert empty.shape == (0, 20) and mf == 0.0


def test_python_refusals_need_no_device():
    f = filter3d.Filter3D(10, device="cpu")
    with pytest.raises(ValueError):
        f.observe(torch.zeros((10, 3), dtype=torch.float64), [R.exact_camera()])
    with pytest.raises(ValueError):
        f.observe(torch.zeros((9, 3)), [R.exact_camera()])
    with pytest.raises(ValueError):
        f.observe(torch.zeros((10, 2)), [R.exact_camera()])
    with pytest.raises(ValueError):
        f.finalize()
    with pytest.raises(ValueError):
        f.remap(torch.zeros(3, dtype=torch.int64))
    s, o = torch.ones((10, 4)), torch.ones(10)
    for bad in (torch.ones(9), torch.ones(10, dtype=torch.float64), torch.ones((10, 1)), torch.ones(10, requires_grad=True)):
        with pytest.raises(ValueError):
            filter3d.smoothed(s, o, bad)
        with pytest.raises(ValueError):
            filter3d.smooth(s, o, bad)
    with pytest.raises(ValueError):
        filter3d.smoothed(torch.ones((10, 3)), o, torch.ones(10))


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
HEADER = "gsrast_amd_filter3d.h"
STRUCTS = {"gsr_filter3d_observe_args": _capi.Filter3dObserveArgs, "gsr_filter3d_finalize_args": _capi.Filter3dFinalizeArgs,
           "gsr_filter3d_args": _capi.Filter3dArgs, "gsr_filter3d_backward_args": _capi.Filter3dBackwardArgs}


def _declared_functions():
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_filter3d_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_filter3d_backward", "gsr_filter3d_finalize", "gsr_filter3d_forward", "gsr_filter3d_observe", "gsr_filter3d_temp_bytes"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in {HEADER} but not exported"
    assert set(_capi.FILTER3D_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES):
        assert not set(_capi.FILTER3D_SIGNATURES) & set(other)
    text = open(os.path.join(ROOT, "include", HEADER)).read()
    assert f"#define GSR_FILTER3D_CAMERA_FLOATS {_capi.GSR_FILTER3D_CAMERA_FLOATS}\n" in text
    assert f"#define GSR_FILTER3D_CAMERA_CHUNK {_capi.GSR_FILTER3D_CAMERA_CHUNK}\n" in text
    assert "0x3EE4F92E" in text


def test_the_structs_are_the_headers_and_the_header_compiles_as_c(tmp_path):
    body = ""
    for cname, cls in STRUCTS.items():
        body += f'printf("{cname} size %zu\\n", sizeof({cname}));'
        body += "".join(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    head = f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{'
    src, exe = tmp_path / "filter3d_abi.c", tmp_path / "filter3d_abi"
    src.write_text(head + body + "int (*o)(gsr_filter3d_observe_args*) = gsr_filter3d_observe; (void)o;"
                   "int (*z)(gsr_filter3d_finalize_args*) = gsr_filter3d_finalize; (void)z;"
                   "int (*f)(gsr_filter3d_args*) = gsr_filter3d_forward; (void)f;"
                   "int (*b)(gsr_filter3d_backward_args*) = gsr_filter3d_backward; (void)b;"
                   "size_t (*t)(int32_t) = gsr_filter3d_temp_bytes; (void)t; return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "filter3d_abi.o")])
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
CALLS = {"observe": (_capi.Filter3dObserveArgs, "gsr_filter3d_observe"), "finalize": (_capi.Filter3dFinalizeArgs, "gsr_filter3d_finalize"),
         "forward": (_capi.Filter3dArgs, "gsr_filter3d_forward"), "backward": (_capi.Filter3dBackwardArgs, "gsr_filter3d_backward")}


def _valid(which):
    a = CALLS[which][0]()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(type(a)), 0, N
    if which == "observe":
        a.position_stride, a.num_cameras = 3, 5
        a.positions, a.cameras, a.min_depth = BASE + 4, BASE + 0x1000, BASE + 0x2000        # (float rows: 4-byte alignment is enough)
    elif which == "finalize":
        a.max_focal = 500.0
        a.min_depth, a.filter, a.temp, a.temp_bytes = BASE, BASE + 0x1000, BASE + 0x2000, _capi.lib().gsr_filter3d_temp_bytes(N)
    else:
        a.scales, a.opacities, a.filter = BASE, BASE + 0x1000, BASE + 0x2000
        if which == "forward":
            a.scales_out, a.opacities_out = BASE + 0x3000, BASE + 0x4000
        else:
            a.dL_dscales_out, a.dL_dopacities_out, a.radii = BASE + 0x3000, BASE + 0x4000, BASE + 0x5000
            a.dL_dscales, a.dL_dopacities = BASE + 0x6000, BASE + 0x7000
    return a


def _set(name, value):
    return lambda a: setattr(a, name, value)


def _set_all(value, *names):
    def go(a):
        for name in names:
            setattr(a, name, value)
    return go


COMMON = {
    "struct_size too small": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) - 8),
    "struct_size too large": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) + 8),
    "struct_size zero": _set("struct_size", 0),
    "a flag": _set("flags", 1),
    "a high flag": _set("flags", 0x80000000),
    "negative N": _set("num_gaussians", -1),
}
REFUSALS = {
    "observe": dict(COMMON, **{
        "negative camera count": _set("num_cameras", -1),
        "stride 2": _set("position_stride", 2), "stride 5": _set("position_stride", 5), "stride 0": _set("position_stride", 0),
        "no positions": _set("positions", None), "no cameras": _set("cameras", None), "no min_depth": _set("min_depth", None),
        "min_depth aliases positions": _set("min_depth", BASE + 4),
    }),
    "finalize": dict(COMMON, **{
        "max_focal zero": _set("max_focal", 0.0), "max_focal negative": _set("max_focal", -1.0),
        "max_focal NaN": _set("max_focal", float("nan")), "max_focal infinite": _set("max_focal", float("inf")),
        "no min_depth": _set("min_depth", None), "no filter": _set("filter", None), "no temp": _set("temp", None),
        "temp too short": _set("temp_bytes", 15), "temp of no bytes": _set("temp_bytes", 0), "temp off a 16-byte boundary": _set("temp", BASE + 0x2008),
        "filter aliases min_depth": _set("filter", BASE),
    }),
    "forward": dict(COMMON, **{
        "no scales": _set("scales", None), "no opacities": _set("opacities", None), "no filter": _set("filter", None),
        "all outputs NULL": _set_all(None, "scales_out", "opacities_out"),
        "scales_out aliases scales": _set("scales_out", BASE), "opacities_out aliases opacities": _set("opacities_out", BASE + 0x1000),
        "opacities_out aliases filter": _set("opacities_out", BASE + 0x2000),
        "scales off a 16-byte boundary": _set("scales", BASE + 4), "scales_out off a 16-byte boundary": _set("scales_out", BASE + 0x3008),
    }),
    "backward": dict(COMMON, **{
        "no scales": _set("scales", None), "no opacities": _set("opacities", None), "no filter": _set("filter", None),
        "no incoming gradient": _set_all(None, "dL_dscales_out", "dL_dopacities_out"),
        "all outputs NULL": _set_all(None, "dL_dscales", "dL_dopacities"),
        "dL_dscales aliases dL_dscales_out": _set("dL_dscales", BASE + 0x3000), "dL_dscales aliases scales": _set("dL_dscales", BASE),
        "dL_dopacities aliases dL_dopacities_out": _set("dL_dopacities", BASE + 0x4000),
        "dL_dopacities aliases opacities": _set("dL_dopacities", BASE + 0x1000),
        "scales off a 16-byte boundary": _set("scales", BASE + 8), "dL_dscales_out off a 16-byte boundary": _set("dL_dscales_out", BASE + 0x3004),
        "dL_dscales off a 16-byte boundary": _set("dL_dscales", BASE + 0x6008),
    }),
}
CASES = [(which, case) for which, cases in REFUSALS.items() for case in cases]


def _refused(fn, a):
    L = _capi.lib()
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert fn(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""


@pytest.mark.parametrize("which,case", CASES)
def test_every_refusal_is_decided_without_a_device(which, case):
    fn = getattr(_capi.lib(), CALLS[which][1])
    a = _valid(which)
    REFUSALS[which][case](a)
    _refused(fn, a)
    # ... and with N == 0 it stays a refusal
    a.num_gaussians = 0 if case != "negative N" else -1
    _refused(fn, a)


def test_null_args_an_empty_scene_and_temp_bytes():
    L = _capi.lib()
    for which, (_, name) in CALLS.items():
        fn = getattr(L, name)
        assert fn(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
        # N == 0: GSR_OK, nothing launched or written — no device needed
        a = _valid(which)
        a.num_gaussians = 0
        assert fn(C.byref(a)) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    # one output, one incoming gradient and no radii are enough; no cameras is no work
    a = _valid("forward")
    a.num_gaussians, a.scales_out = 0, None
    assert L.gsr_filter3d_forward(C.byref(a)) == _capi.GSR_OK
    a = _valid("backward")
    a.num_gaussians, a.dL_dscales_out, a.radii, a.dL_dopacities = 0, None, None, None
    assert L.gsr_filter3d_backward(C.byref(a)) == _capi.GSR_OK
    a = _valid("observe")
    a.num_cameras, a.cameras = 0, None
    assert L.gsr_filter3d_observe(C.byref(a)) == _capi.GSR_OK            # (N > 0: still nothing to launch)
    a = _valid("observe")
    a.num_cameras = 65536 * _capi.GSR_FILTER3D_CAMERA_CHUNK
    assert L.gsr_filter3d_observe(C.byref(a)) == _capi.GSR_ERR_TOO_LARGE
    assert L.gsr_filter3d_temp_bytes(-1) == 0
    for n in (0, 1, 1 << 20, (1 << 31) - 1):
        t = L.gsr_filter3d_temp_bytes(n)
        assert t >= 4 and t % 16 == 0
