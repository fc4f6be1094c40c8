"""CPU: the two operators of the normal-consistency loss (include/gsrast_amd_normals.h). The float32 restatements of
tests/normals_ref.py by hand, its float64 references against central finite differences and against the restatements, what a
rotated camera and a fronto-parallel plane give, the blindness guards of the seeded cases tests/test_gpu_normals.py uses; the
eleventh header against its ctypes table; every refusal of the four calls without a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import normals_ref as R
from helpers import ROOT

from gsrast_amd import _capi

F = np.float32
PROFILES = R.PROFILES
IDENTITY_VIEW = np.ascontiguousarray(np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 5], [0, 0, 0, 1]], F).T.reshape(-1))   # t = m + (0, 0, 5)


# ---- the restatements by hand ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", PROFILES)
def test_gaussian_normals_by_hand(semantics):
    """R = I (a unit real quaternion) and t = m + (0, 0, 5): the normal is the shortest axis' unit vector, negated where it has a
    positive product with t."""
    rows = [  # scales, mean, quaternion -> normal
        ((0.1, 1.0, 1.0), (1.0, 0.0, 0.0), (1, 0, 0, 0), (-1, 0, 0)),       # x shortest, d = 1 > 0: flipped
        ((0.1, 1.0, 1.0), (-1.0, 0.0, 0.0), (1, 0, 0, 0), (1, 0, 0)),       # d = -1: not flipped
        ((1.0, 0.1, 1.0), (0.0, 2.0, 0.0), (1, 0, 0, 0), (0, -1, 0)),       # y shortest
        ((1.0, 0.1, 1.0), (0.0, -2.0, 0.0), (1, 0, 0, 0), (0, 1, 0)),
        ((1.0, 1.0, 0.1), (0.0, 0.0, 0.0), (1, 0, 0, 0), (0, 0, -1)),       # z shortest, d = 5
        ((1.0, 1.0, 0.1), (0.0, 0.0, -9.0), (1, 0, 0, 0), (0, 0, 1)),       # behind the camera: d = -4
        ((0.2, 0.2, 0.2), (1.0, 1.0, 0.0), (1, 0, 0, 0), (-1, 0, 0)),       # a tie keeps the lower index
        ((0.5, 0.2, 0.2), (1.0, 1.0, 0.0), (1, 0, 0, 0), (0, -1, 0)),
        ((0.1, 1.0, 1.0), (0.0, 1.0, 0.0), (1, 0, 0, 0), (1, 0, 0)),        # d = 0 is not > 0: not flipped
        ((np.nan, 1.0, 0.5), (1.0, 0.0, 0.0), (1, 0, 0, 0), (-1, 0, 0)),    # a NaN in s0 is never undercut: axis 0
        ((0.1, 1.0, 1.0), (1.0, 0.0, 0.0), (2, 0, 0, 0), None),             # an unnormalised quaternion: see below
        ((0.1, 1.0, 1.0), (1.0, 0.0, 0.0), (0, 0, 0, 0), None),             # a zero quaternion: see below
    ]
    means = np.array([r[1] + (1.0,) for r in rows], F)
    scales = np.array([r[0] + (np.e,) for r in rows], F)
    quats = np.array([r[2] for r in rows], F)
    got, dec = R.gaussian_normals_f32(means, scales, quats, IDENTITY_VIEW, semantics)
    for i, r in enumerate(rows):
        if r[3] is not None:
            assert np.array_equal(got[i], np.array(r[3], F)), (i, got[i])
    assert list(dec["axis"][:10]) == [0, 0, 1, 1, 2, 2, 0, 1, 0, 0]
    assert list(dec["flipped"][:9]) == [True, False, True, False, True, False, True, True, False]
    if semantics == "gscuda":
        # the reference profile normalises q: the same normal; a zero quaternion has no direction: zeros
        assert np.array_equal(got[10], np.array((-1, 0, 0), F)) and not dec["valid"][11] and (got[11].view(np.uint32) == 0).all()
    else:
        # upstream's R of q = (2, 0, 0, 0) is still I (only x, y, z enter its entries), and of q = 0 too
        assert np.array_equal(got[10], np.array((-1, 0, 0), F)) and np.array_equal(got[11], np.array((-1, 0, 0), F))
    # a rotation by 90 degrees about z takes the x axis to y: the normal of an x-shortest Gaussian at +y is (0, -1, 0)
    s = np.sqrt(0.5)
    got, _ = R.gaussian_normals_f32(np.array([[0, 3, 0, 1]], F), np.array([[0.1, 1, 1, np.e]], F), np.array([[s, 0, 0, s]], F), IDENTITY_VIEW,
                                    semantics)
    assert np.allclose(got[0], (0, -1, 0), atol=1e-6)


@pytest.mark.parametrize("semantics", PROFILES)
def test_depth_normals_by_hand(semantics):
    tan = (0.5, 0.25)
    flat, dec = R.depth_normals_f32(np.full((3, 3), 2.0, F), tan, semantics)
    assert np.array_equal(flat[:, 1, 1], np.array((0, 0, -1), F)) and dec["valid"].sum() == 1 and not dec["flipped"].any()
    border = np.ones((3, 3), bool)
    border[1, 1] = False
    assert (flat[:, border].view(np.uint32) == 0).all()
    # the centre's own depth is not read; a hole among the four neighbours leaves zeros
    d = np.full((3, 3), 2.0, F)
    d[1, 1] = np.nan
    assert np.array_equal(R.depth_normals_f32(d, tan, semantics)[0].view(np.uint32), flat.view(np.uint32))
    for hole in R.HOLES:
        d = np.full((3, 3), 2.0, F)
        d[0, 1] = hole
        out, dec = R.depth_normals_f32(d, tan, semantics)
        assert (out.view(np.uint32) == 0).all() and not dec["valid"].any()
    # one pixel in plain Python floats: depths 1 (left), 3 (right), 2 (up and down)
    d = np.array([[9, 2, 9], [1, 9, 3], [9, 2, 9]], F)
    out, dec = R.depth_normals_f32(d, tan, semantics)
    off = 1.0 if semantics == "inria" else 0.0
    ray = lambda i, t: ((2.0 * i + off) / 3.0 - 1.0) * t
    rx, rxl, rxr, ry, ryu, ryd = ray(1, tan[0]), ray(0, tan[0]), ray(2, tan[0]), ray(1, tan[1]), ray(0, tan[1]), ray(2, tan[1])
    dv = np.array([rx * 2 - rx * 2, ryd * 2 - ryu * 2, 0.0])
    dh = np.array([rxr * 3 - rxl * 1, ry * 3 - ry * 1, 2.0])
    c = np.cross(dv, dh)
    c = -c if c @ np.array([rx, ry, 1.0]) > 0 else c
    assert np.allclose(out[:, 1, 1], c / np.linalg.norm(c), atol=1e-6) and out[2, 1, 1] < 0
    # below three pixels in either direction there is no interior
    for shape in ((1, 1), (2, 7), (7, 2)):
        assert (R.depth_normals_f32(np.full(shape, 2.0, F), tan, semantics)[0].view(np.uint32) == 0).all()


# ---- the float64 references -------------------------------------------------------------------------------------------------------------
def _views(semantics):
    return R.random_view(3, mirrored=(semantics == "gscuda"))


@pytest.mark.parametrize("semantics", PROFILES)
def test_gaussian_reference_against_finite_differences(semantics):
    means, scales, quats = R.gaussian_case(300, seed=1, edges=False)
    view = _views(semantics)
    _, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    assert dec["valid"].all()
    g = R.seed_gradient((300, 3))
    ref = R.gaussian_gradients64(quats, view, g, dec, semantics)
    v64 = torch.from_numpy(view.astype(np.float64))

    def loss_rows(q):
        with torch.no_grad():
            return (R.gaussian_normals64(torch.from_numpy(q), v64, dec, semantics).numpy() * g.astype(np.float64)).sum(1)
    base = quats.astype(np.float64)
    for k in range(4):
        h = 1e-6
        up, dn = base.copy(), base.copy()
        up[:, k] += h
        dn[:, k] -= h
        fd = (loss_rows(up) - loss_rows(dn)) / (2 * h)
        scale = np.maximum(np.abs(ref).max(1), 1e-12)
        assert (np.abs(fd - ref[:, k]) <= 1e-6 * scale + 1e-9).all(), (k, float((np.abs(fd - ref[:, k]) / scale).max()))
    if semantics == "gscuda":          # its preprocess normalises q: the normal does not change along q
        assert np.abs((ref * base).sum(1)).max() <= 1e-12 * np.abs(ref).max()
    else:
        assert np.abs((ref * base).sum(1)).max() > 1e-3


@pytest.mark.parametrize("semantics", PROFILES)
def test_depth_reference_against_finite_differences(semantics):
    depth = R.depth_case(7, 9, seed=2)
    _, dec = R.depth_normals_f32(depth, R.TAN_FOV, semantics)
    assert dec["valid"].sum() >= 10
    g = R.seed_gradient((3, 7, 9), seed=6)
    total, terms = R.depth_gradients64(depth, g, R.TAN_FOV, semantics, dec)
    assert np.array_equal(total, ((terms[0] + terms[1]) + terms[2]) + terms[3])
    base = np.where(np.isfinite(depth), depth, 1.0).astype(np.float64)

    def loss(d):
        t = torch.from_numpy(d)
        with torch.no_grad():
            return float((R.depth_normals64(t, t, t, t, R.TAN_FOV, semantics, dec).numpy() * g.astype(np.float64)).sum())
    for y in range(7):
        for x in range(9):
            h = 1e-6
            up, dn = base.copy(), base.copy()
            up[y, x] += h
            dn[y, x] -= h
            fd = (loss(up) - loss(dn)) / (2 * h)
            assert abs(fd - total[y, x]) <= 1e-6 * max(np.abs(terms[:, y, x]).sum(), 1.0), (y, x, fd, total[y, x])
    # each term belongs to one neighbour: a pixel whose neighbour is not valid gets nothing from it
    ok = dec["valid"]
    assert (terms[0][1:][~ok[:-1]] == 0).all() and (terms[3][:-1][~ok[1:]] == 0).all()
    assert (terms[1][:, 1:][~ok[:, :-1]] == 0).all() and (terms[2][:, :-1][~ok[:, 1:]] == 0).all()
    assert (terms[0][0] == 0).all() and (terms[1][:, 0] == 0).all() and (terms[2][:, -1] == 0).all() and (terms[3][-1] == 0).all()
    assert all((np.abs(t) > 0).sum() >= 5 for t in terms)


@pytest.mark.parametrize("semantics", PROFILES)
def test_float32_restatements_are_the_float64_functions_to_rounding(semantics):
    """The Gaussian normal is a dozen float32 operations on entries of size 1: 1e-6. The depth normal loses what the differences of
    neighbouring depths cancel: depths of about 4 with 2^-24 relative rounding against differences of 0.02 and more (the case's
    noise alone), 4 x 6e-8 / 0.02 = 1.2e-5 per difference and a handful of them: 2e-4."""
    means, scales, quats = R.gaussian_case(1000, seed=2, edges=False)
    view = _views(semantics)
    n32, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    n64 = R.gaussian_normals64(torch.from_numpy(quats.astype(np.float64)), torch.from_numpy(view.astype(np.float64)), dec, semantics).numpy()
    err = float(np.abs(n32 - n64).max())
    print(f"{semantics}: Gaussian normals, max |f32 - f64| = {err:.2e}")
    assert err <= 1e-6 and np.allclose(np.linalg.norm(n64, axis=1), 1.0, atol=1e-12)
    depth = R.depth_case(64, 48, seed=1)
    d32, dec = R.depth_normals_f32(depth, R.TAN_FOV, semantics)
    t = torch.from_numpy(np.where(np.isfinite(depth), depth, 1.0).astype(np.float64))
    d64 = R.depth_normals64(t, t, t, t, R.TAN_FOV, semantics, dec).numpy()
    err = float(np.abs(d32 - d64).max())
    print(f"{semantics}: depth normals, max |f32 - f64| = {err:.2e}")
    assert err <= 2e-4
    # every valid normal faces the camera: a negative product with the pixel's ray
    ys, xs = np.nonzero(dec["valid"])
    rays = np.stack([R.ndc(xs, 48, semantics, np.float64) * R.TAN_FOV[0], R.ndc(ys, 64, semantics, np.float64) * R.TAN_FOV[1], np.ones(len(xs))])
    assert ((d64[:, ys, xs] * rays).sum(0) < 1e-9).all()


@pytest.mark.parametrize("semantics", PROFILES)
def test_a_tilted_plane_has_its_analytic_normal(semantics):
    """The float32 depth of a plane rounds each depth by 2^-24 x 4 = 2.4e-7 over a two-pixel baseline of 0.04 and more in space: the
    float64 reference of the ROUNDED depths is within 10 x 2.4e-7 / 0.04 = 6e-5 of the plane's normal; of the unrounded depths,
    exact to 1e-9."""
    normal = np.array([0.3, -0.2, -1.0])
    normal /= np.linalg.norm(normal)
    exact = R.plane_depth(33, 65, normal, -4.0, R.TAN_FOV, semantics)
    assert (exact > 2).all() and (exact < 8).all()
    _, dec = R.depth_normals_f32(exact.astype(F), R.TAN_FOV, semantics)
    assert dec["valid"][1:-1, 1:-1].all()
    t = torch.from_numpy(exact)
    n = R.depth_normals64(t, t, t, t, R.TAN_FOV, semantics, dec).numpy()[:, 1:-1, 1:-1]
    assert np.abs(n - normal[:, None, None]).max() <= 1e-9
    t = torch.from_numpy(exact.astype(F).astype(np.float64))
    n = R.depth_normals64(t, t, t, t, R.TAN_FOV, semantics, dec).numpy()[:, 1:-1, 1:-1]
    assert np.abs(n - normal[:, None, None]).max() <= 6e-5


@pytest.mark.parametrize("semantics", PROFILES)
def test_rotating_the_camera_rotates_the_normal(semantics):
    """V' = Q V for a rotation Q: W' = Q W and t' = Q t, so n_v' = Q n_v, and the flip's product is the same number. Rows whose
    product is within 1e-3 of zero may flip with the rounding and are left out."""
    means, scales, quats = R.gaussian_case(500, seed=3, edges=False)
    view = _views(semantics)
    a = 0.7
    Q = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, np.cos(0.4), -np.sin(0.4)], [0, np.sin(0.4), np.cos(0.4)]])
    V = view.astype(np.float64).reshape(4, 4).T
    V2 = V.copy()
    V2[:3] = Q @ V[:3]
    view2 = np.ascontiguousarray(V2.T.reshape(-1).astype(F))
    n1, d1 = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    n2, d2 = R.gaussian_normals_f32(means, scales, quats, view2, semantics)
    t = (V[:3, :3] @ means[:, :3].T.astype(np.float64)).T + V[:3, 3]
    keep = np.abs((n1.astype(np.float64) * t).sum(1)) > 1e-3
    assert keep.sum() >= 450 and np.array_equal(d1["flipped"][keep], d2["flipped"][keep])
    assert np.abs(n2[keep] - n1[keep].astype(np.float64) @ Q.T).max() <= 2e-6


@pytest.mark.parametrize("semantics", PROFILES)
def test_loss_is_zero_on_a_fronto_parallel_plane(semantics):
    """Flat splats in a plane z = const of the camera, their shortest axis along z: every Gaussian normal is (0, 0, -1) exactly, so
    is their blend at full opacity, the plane's depth is constant, and 1 - N_r . N_d is exactly 0 on the interior."""
    n = 64
    rng = np.random.default_rng(4)
    means = np.ones((n, 4), F)
    means[:, :2] = rng.uniform(-2, 2, (n, 2))
    means[:, 2] = 0.0
    scales = np.tile(np.array([0.3, 0.4, 0.01, np.e], F), (n, 1))
    # rotations about z only: the z axis stays the z axis
    ang = rng.uniform(0, 6.28, n)
    quats = np.stack([np.cos(ang / 2), 0 * ang, 0 * ang, np.sin(ang / 2)], 1).astype(F)
    normals, dec = R.gaussian_normals_f32(means, scales, quats, IDENTITY_VIEW, semantics)
    assert (dec["axis"] == 2).all() and dec["flipped"].all() and np.array_equal(normals, np.tile(np.array([0, 0, -1], F), (n, 1)))
    weights = rng.dirichlet(np.ones(n), size=(5, 7)).astype(np.float64)          # any blend weights that sum to one
    n_r = np.einsum("yxi,ic->cyx", weights, normals.astype(np.float64))
    n_d, _ = R.depth_normals_f32(np.full((5, 7), 5.0, F), R.TAN_FOV, semantics)
    loss = 1.0 - (n_r * n_d).sum(0)
    assert np.abs(loss[1:-1, 1:-1]).max() <= 1e-15 and (loss[0] == 1).all()


# ---- blindness guards ---------------------------------------------------------------------------------------------------------------------
GPU_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
GPU_SHAPES = ((1, 1), (2, 7), (3, 3), (3, 65), (65, 3), (17, 33), (64, 48), (67, 131), (4, 64), (5, 65), (3, 63), (8, 128), (9, 129))


@pytest.mark.parametrize("semantics", PROFILES)
def test_seeded_cases_hold_every_case(semantics):
    view = _views(semantics)
    means, scales, quats = R.gaussian_case(1000, seed=0)
    _, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    n = 1000
    for a in range(3):
        assert (dec["axis"] == a).sum() >= n // 10, a
    ok = dec["valid"]
    assert (dec["flipped"] & ok).sum() >= n // 5 and (~dec["flipped"] & ok).sum() >= n // 5
    assert 1 <= (~ok).sum() <= 10
    V = view.astype(np.float64).reshape(4, 4).T
    tz = (V[:3, :3] @ means[:, :3].T.astype(np.float64)).T[:, 2] + V[2, 3]
    assert (tz < 0).sum() >= 20, "means behind the camera"
    means, scales, quats = R.gaussian_case(1000, seed=21, edges=False)
    _, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    assert dec["valid"].all() and dec["flipped"].sum() >= 200 and (~dec["flipped"]).sum() >= 200
    for h, w in ((64, 48), (67, 131), (17, 33)):
        _, dec = R.depth_normals_f32(R.depth_case(h, w, seed=1), R.TAN_FOV, semantics)
        inner = dec["interior"].sum()
        holes = (dec["interior"] & ~dec["finite"]).sum()
        print(f"{semantics} {h} x {w}: {holes} of {inner} interior pixels have an invalid neighbour; {int(dec['flipped'].sum())} flipped")
        assert holes >= 0.1 * inner and dec["finite"].sum() >= 0.5 * inner    # the depth backward's bound: at most 1 % of the pixels may use its looser branch
    for h, w in ((64, 48), (67, 131)):
        depth = R.depth_case(h, w, seed=1)
        total, terms = R.depth_gradients64(depth, R.seed_gradient((3, h, w), seed=h), R.TAN_FOV, semantics)
        loose = np.abs(total) < 2.0 ** -20 * np.abs(terms).sum(0)
        assert (loose & (np.abs(terms).sum(0) > 0)).sum() <= 0.01 * h * w


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
HEADER = "gsrast_amd_normals.h"
STRUCTS = {"gsr_gaussian_normals_args": _capi.GaussianNormalsArgs, "gsr_gaussian_normals_backward_args": _capi.GaussianNormalsBackwardArgs,
           "gsr_depth_normals_args": _capi.DepthNormalsArgs, "gsr_depth_normals_backward_args": _capi.DepthNormalsBackwardArgs}
FUNCTIONS = {"gsr_gaussian_normals_forward": "gsr_gaussian_normals_args", "gsr_gaussian_normals_backward": "gsr_gaussian_normals_backward_args",
             "gsr_depth_normals_forward": "gsr_depth_normals_args", "gsr_depth_normals_backward": "gsr_depth_normals_backward_args"}


def test_library_exports_every_symbol_the_normals_header_declares():
    L = _capi.lib()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", HEADER)).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(FUNCTIONS)
    for n in names:
        assert hasattr(L, n), f"{n} declared in {HEADER} but not exported"
    assert set(_capi.NORMALS_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES,
                  _capi.DISTORTION_SIGNATURES):
        assert not set(_capi.NORMALS_SIGNATURES) & set(other)
    build = open(os.path.join(ROOT, "gsrast_amd", "build.py")).read()
    assert HEADER in build, "the build does not watch the header"


def test_the_structs_are_the_headers_and_the_header_compiles_as_c(tmp_path):
    body = ""
    for cname, cls in STRUCTS.items():
        body += f'printf("{cname} size %zu\\n", sizeof({cname}));'
        body += "".join(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_)
    head = f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\nint main(void){{'
    src, exe = tmp_path / "normals_abi.c", tmp_path / "normals_abi"
    pointers = "".join(f"int (*f{i})({arg}*) = {fn}; (void)f{i};" for i, (fn, arg) in enumerate(FUNCTIONS.items()))
    src.write_text(head + body + pointers + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "normals_abi.o")])
    src.write_text(head + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {tuple(line.split()[:2]): int(line.split()[2]) for line in subprocess.check_output([str(exe)], text=True).splitlines()}
    for cname, cls in STRUCTS.items():
        assert got[(cname, "size")] == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert got[(cname, f)] == getattr(cls, f).offset, (cname, f)


# ---- the error contract, without a device -----------------------------------------------------------------------------------------------
BASE = 0x10000000                 # addresses nothing dereferences: every case is decided before any HIP call


def _valid(name):
    a = STRUCTS[FUNCTIONS[name]]()
    a.struct_size, a.flags = C.sizeof(type(a)), 0
    if "gaussian" in name:
        a.num_gaussians = 100
        a.means3D, a.scales, a.rotations, a.view_matrix = BASE, BASE + 0x1000, BASE + 0x2000, BASE + 0x3000
        if name.endswith("backward"):
            a.dL_dnormals, a.radii, a.dL_drotations = BASE + 0x4000, BASE + 0x5000, BASE + 0x6000
        else:
            a.normals = BASE + 0x4004             # (float[N][3]: four-byte alignment is enough)
    else:
        a.width, a.height, a.tan_fovx, a.tan_fovy = 64, 48, 0.5, 0.4
        a.depth = BASE
        if name.endswith("backward"):
            a.dL_dnormals, a.dL_ddepth = BASE + 0x10000, BASE + 0x40000
        else:
            a.normals = BASE + 0x10000
    return a


def _set(name, value):
    return lambda a: setattr(a, name, value)


_SHARED = {
    "struct_size too small": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) - 8),
    "struct_size too large": lambda a: setattr(a, "struct_size", C.sizeof(type(a)) + 8),
    "struct_size zero": _set("struct_size", 0),
    "an unknown flag": _set("flags", _capi.GSR_FLAG_PROFILE),
    "an unknown flag beside the profile's": _set("flags", _capi.GSR_FLAG_SEMANTICS_INRIA | 0x80000000),
}
_GAUSSIAN = dict(_SHARED, **{
    "negative N": _set("num_gaussians", -1), "no means3D": _set("means3D", None), "no scales": _set("scales", None),
    "no rotations": _set("rotations", None), "no view_matrix": _set("view_matrix", None),
    "means3D off a 16-byte boundary": _set("means3D", BASE + 4), "scales off a 16-byte boundary": _set("scales", BASE + 0x1008),
    "rotations off a 16-byte boundary": _set("rotations", BASE + 0x200C)})
_DEPTH = dict(_SHARED, **{
    "width zero": _set("width", 0), "height negative": _set("height", -4), "tan_fovx zero": _set("tan_fovx", 0.0),
    "tan_fovx NaN": _set("tan_fovx", float("nan")), "tan_fovy negative": _set("tan_fovy", -0.4),
    "tan_fovy infinite": _set("tan_fovy", float("inf")), "no depth": _set("depth", None)})
REFUSALS = {
    "gsr_gaussian_normals_forward": dict(_GAUSSIAN, **{"no normals": _set("normals", None)}),
    "gsr_gaussian_normals_backward": dict(_GAUSSIAN, **{"no dL_dnormals": _set("dL_dnormals", None), "no dL_drotations": _set("dL_drotations", None),
                                                        "dL_drotations off a 16-byte boundary": _set("dL_drotations", BASE + 0x6008)}),
    "gsr_depth_normals_forward": dict(_DEPTH, **{"no normals": _set("normals", None), "normals aliases depth": _set("normals", BASE)}),
    "gsr_depth_normals_backward": dict(_DEPTH, **{"no dL_dnormals": _set("dL_dnormals", None), "no dL_ddepth": _set("dL_ddepth", None),
                                                  "dL_ddepth aliases depth": _set("dL_ddepth", BASE),
                                                  "dL_ddepth aliases dL_dnormals": _set("dL_ddepth", BASE + 0x10000)}),
}


@pytest.mark.parametrize("name,case", [(n, c) for n in REFUSALS for c in REFUSALS[n]])
def test_every_refusal_is_decided_without_a_device(name, case):
    L = _capi.lib()
    a = _valid(name)
    REFUSALS[name][case](a)
    tries = [a]
    if "gaussian" in name and case != "negative N":          # ... and with N == 0 it stays a refusal
        b = _valid(name)
        REFUSALS[name][case](b)
        b.num_gaussians = 0
        tries.append(b)
    for t in tries:
        assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
        assert getattr(L, name)(C.byref(t)) == _capi.GSR_ERR_INVALID_ARG
        assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_hip_error() == b""


def test_null_args_too_many_blocks_and_an_empty_scene():
    L = _capi.lib()
    for name in FUNCTIONS:
        assert getattr(L, name)(None) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    # N == 0: GSR_OK, nothing launched or written — no device needed; radii may be NULL
    for name in ("gsr_gaussian_normals_forward", "gsr_gaussian_normals_backward"):
        a = _valid(name)
        a.num_gaussians, a.flags = 0, _capi.GSR_FLAG_SEMANTICS_INRIA
        if name.endswith("backward"):
            a.radii = None
        assert getattr(L, name)(C.byref(a)) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    # more blocks of 64 x 4 pixels than a grid holds
    for name in ("gsr_depth_normals_forward", "gsr_depth_normals_backward"):
        a = _valid(name)
        a.width, a.height = 2 ** 31 - 1, 2 ** 31 - 1
        assert getattr(L, name)(C.byref(a)) == _capi.GSR_ERR_TOO_LARGE and L.gsr_last_error() == _capi.GSR_ERR_TOO_LARGE
