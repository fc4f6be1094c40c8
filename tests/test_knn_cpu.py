"""CPU: the reference of gsr_knn_mean_dist2 (tests/knn_ref.py) by hand and against float64; the C ABI's second table
(_capi.INIT_SIGNATURES, include/gsrast_amd_init.h) held to the same two contract tests as the first one in
tests/test_capi_cpu.py; ply.read_points_ply; the Python refusals; and the guards of the scenes tests/test_gpu_knn.py runs:
conditions that make a search along a sorted order alone give wrong results on them. No GPU call is made."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import knn_ref as R
from helpers import ROOT

from gsrast_amd import _capi

F = np.float32
LEAF, NODE = _capi.GSR_KNN_LEAF, _capi.GSR_KNN_NODE
BLOCK = LEAF * NODE


# ---- the scenes (seeded; shared with tests/test_gpu_knn.py, each reference computed once per process) ----
def _uniform(n, seed=1):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, (n, 3)).astype(F)


def _lattice():
    g = np.arange(20, dtype=F)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)


def _coincident():
    """Clusters of 2, 3, 4 and 7 coincident points among 1000 others, in shuffled rows."""
    rng = np.random.default_rng(5)
    p = _uniform(1000, 6)
    extra = [np.repeat(p[i:i + 1], copies - 1, axis=0) for i, copies in ((3, 2), (100, 3), (555, 4), (999, 7))]
    p = np.concatenate([p] + extra)
    return p[rng.permutation(p.shape[0])]


def _plane():
    p = _uniform(4097, 7)
    p[:, 2] = F(0.5)
    return p


def _diagonal_line():
    t = np.random.default_rng(8).uniform(-1.0, 1.0, 1000).astype(F)
    return np.stack([t, F(2) * t, F(-0.5) * t], axis=1).astype(F)


def _axis_line():
    p = np.zeros((1000, 3), F)
    p[:, 1] = np.random.default_rng(9).uniform(-3.0, 3.0, 1000).astype(F)
    p[:, 0], p[:, 2] = F(1.25), F(-7.0)
    return p


def _clusters_and_outlier():
    """Two tight clusters 400 apart and one outlier at 9000: with 10 bits an axis both clusters fall into a few cells."""
    rng = np.random.default_rng(10)
    a = rng.normal(0.0, 1.0, (8192, 3)).astype(F)
    b = (rng.normal(0.0, 1.0, (8192, 3)) + np.array([400.0, 0.0, 0.0])).astype(F)
    return np.concatenate([a, b, np.array([[9000.0, 9000.0, 9000.0]], F)])


def _offset():
    """Coordinates near 1e4, where a float32 ulp is 2^-10: the leaf boxes are a few ulps wide and distances tie."""
    return (np.random.default_rng(11).uniform(0.0, 1.0, (4097, 3)) + 1.0e4).astype(F)


SCENES = {
    "uniform": lambda: _uniform(16384),
    "lattice": _lattice,
    "identical": lambda: np.tile(np.array([[0.3, -1.2, 2.5]], F), (4097, 1)),
    "coincident": _coincident,
    "plane": _plane,
    "diagonal_line": _diagonal_line,
    "axis_line": _axis_line,
    "clusters_and_outlier": _clusters_and_outlier,
    "offset": _offset,
}
LARGE = ("uniform", "plane", "clusters_and_outlier")
SIZES = sorted({1, 2, 3, 4, 5, LEAF - 1, LEAF, LEAF + 1, 2 * LEAF + 1, BLOCK - 1, BLOCK, BLOCK + 1, min(3 * BLOCK + 17, 16385)})


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene `name`, or the `uniform_<n>` of a size; read only."""
    p = _uniform(int(name[8:]), 100 + int(name[8:])) if name.startswith("uniform_") else SCENES[name]()
    assert p.dtype == F and p.ndim == 2 and p.shape[1] == 3 and p.shape[0] <= 16385 and np.isfinite(p).all()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def reference_of(name):
    """(mean_dist2 float32 [n], the rows of the true neighbours [n,k]) of a scene by brute force; read only."""
    p = scene(name)
    d2, idx = R.nearest(p, F)
    mean = R.mean_of(d2, p.shape[0])
    assert mean.dtype == F
    mean.setflags(write=False)
    idx.setflags(write=False)
    return mean, idx


# ---- the reference by hand ----
def test_reference_on_five_collinear_points():
    x = np.array([0.0, 1.0, 3.0, 7.0, 15.0], F)
    p = np.stack([x, np.zeros(5, F), np.zeros(5, F)], axis=1)
    d2, idx = R.nearest(p)
    assert d2.tolist() == [[1, 9, 49], [1, 4, 36], [4, 9, 16], [16, 36, 49], [64, 144, 196]]
    assert np.sort(idx, axis=1).tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [1, 2, 3]]
    want = [F(F(1 + 9) + F(49)) / F(3), F(41) / F(3), F(29) / F(3), F(101) / F(3), F(404) / F(3)]
    assert R.mean_dist2(p).tolist() == [float(w) for w in want]
    assert R.mean_dist2(p).dtype == F


def test_reference_with_fewer_than_four_points():
    p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [0.0, 0.0, 1.0]], F)
    one = R.mean_dist2(p[:1])
    assert one.tolist() == [0.0] and not np.signbit(one[0]) and one.dtype == F
    assert R.mean_dist2(p[:2]).tolist() == [25.0, 25.0]                                  # b0
    assert R.mean_dist2(p[:3]).tolist() == [(1.0 + 25.0) / 2, (25.0 + 26.0) / 2, (1.0 + 26.0) / 2]      # (b0 + b1) / 2


def test_reference_counts_a_duplicate_as_a_neighbour_at_distance_zero():
    p = np.array([[1.0, 2.0, 3.0]] * 4 + [[1.0, 2.0, 5.0], [9.0, 2.0, 3.0]], F)
    got = R.mean_dist2(p)
    assert got[:4].tolist() == [0.0] * 4                         # three other copies each
    assert got[4] == F(F(4 + 4) + F(4)) / F(3)                   # three of the four copies, 2 away
    assert got[5] == F(64)                                       # (64 + 64 + 64) / 3


def test_float32_reference_against_float64():
    """Relative 8 * 2^-24 of the float64 value. Derived: each squared difference carries 3 roundings (the difference, which is
    exact in float64 up to 2^-53, and the product: at most (1 + u)^3 with u = 2^-24), the sum of three 2 more, the mean's sum
    2 and its division 1: (1 + u)^8 at most on every term, all terms non-negative, so no cancellation. The k-th smallest of
    values each perturbed by a relative e moves by at most e. Holds where nothing underflows: every non-zero d2 > 1e-20."""
    for name in ("uniform_2000", "coincident", "offset"):
        p = scene(name)
        d32, _ = R.nearest(p, F)
        d64, _ = R.nearest(p, np.float64)
        assert (d32[d32 > 0] > 1e-20).all() and ((d32 == 0) == (d64 == 0)).all()
        m32, m64 = R.mean_of(d32, p.shape[0]), R.mean_of(d64, p.shape[0])
        assert m32.dtype == F and m64.dtype == np.float64
        err = np.abs(m32.astype(np.float64) - m64)
        worst = (err[m64 > 0] / m64[m64 > 0]).max()
        print(f"{name}: worst relative error {worst * 2 ** 24:.2f} * 2^-24")
        assert (err <= 8.0 * 2.0 ** -24 * m64).all(), name


# ---- the scenes' guards ----
@pytest.mark.parametrize("name", LARGE)
def test_large_scenes_defeat_a_search_along_the_sorted_order(name):
    """Conditions, not measurements, on the test's OWN 30-bit Morton order: at least 10 % of the points have a true
    neighbour more than 64 places away (a window of a leaf on either side misses it), and in the two scenes of 16 K points
    at least 1 % have one more than 4096 places away (so does a window of a whole node on either side)."""
    p = scene(name)
    away = R.farthest_neighbour_places(p, reference_of(name)[1])
    print(f"{name}: {100 * (away > 64).mean():.1f} % beyond 64 places, {100 * (away > 4096).mean():.1f} % beyond 4096")
    assert (away > 64).mean() >= 0.10
    if name != "plane":
        assert p.shape[0] >= 16384 and (away > 4096).mean() >= 0.01


def test_scenes_hold_what_their_names_say():
    ext = lambda name: np.ptp(scene(name), axis=0)
    assert (ext("plane") > 0).tolist() == [True, True, False]
    assert (ext("axis_line") > 0).tolist() == [False, True, False] and (ext("diagonal_line") > 0).all()
    assert ext("identical").tolist() == [0, 0, 0] and scene("identical").shape[0] == 4097
    _, counts = np.unique(scene("coincident"), axis=0, return_counts=True)
    assert sorted(counts[counts > 1].tolist()) == [2, 3, 4, 7]
    mean, _ = reference_of("lattice")
    assert scene("lattice").shape[0] == 8000 and (mean == 1.0).all()                    # (three of up to six neighbours at 1)
    far = scene("clusters_and_outlier")
    assert far.shape[0] == 16385 and far[-1].tolist() == [9000.0] * 3
    assert np.unique(scene("offset")[:, 0]).size < 1100                                  # (2^-10 apart in [1e4, 1e4 + 1])
    assert SIZES[-1] == min(3 * BLOCK + 17, 16385) and len(SIZES) == 13


# ---- the C ABI: the second table against its header, and the error contract of its status-returning calls ----
def _declared_functions():
    text = open(os.path.join(ROOT, "include", "gsrast_amd_init.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_init_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert len(names) >= 2
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_init.h but not exported"
    assert set(_capi.INIT_SIGNATURES) == set(names), "ctypes table and header disagree"
    assert not set(_capi.INIT_SIGNATURES) & set(_capi.SIGNATURES)


def test_python_constants_are_the_init_headers(tmp_path):
    import subprocess
    names = sorted(k for k in vars(_capi) if k.startswith("GSR_KNN_"))
    assert {"GSR_KNN_LEAF", "GSR_KNN_NODE"} <= set(names)
    body = "".join(f'printf("{k} %lld\\n", (long long)({k}));' for k in names)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include "gsrast_amd_init.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for k in names:
        assert int(got[k]) == int(getattr(_capi, k)), k


_AT = 0x10000                                               # an invented, 16-byte aligned address: only in calls of ZERO elements
_INVALID = _capi.GSR_ERR_INVALID_ARG
_forward_nulls = lambda: (C.byref(_capi.ForwardArgs(struct_size=C.sizeof(_capi.ForwardArgs))),)
# name -> (arguments that are refused, the code, arguments of a success that makes no HIP call). No row reaches a HIP call.
INIT_ERROR_CONTRACT = {
    "gsr_knn_mean_dist2": ((1, None, None, None, None), _INVALID, (0, None, None, None, None)),
}


def test_the_init_error_contract_table_names_every_status_returning_entry_point():
    derived = {name for name, (res, _) in _capi.INIT_SIGNATURES.items() if res is C.c_int}
    assert derived == set(INIT_ERROR_CONTRACT), sorted(derived ^ set(INIT_ERROR_CONTRACT))


@pytest.mark.parametrize("name", sorted(INIT_ERROR_CONTRACT))
def test_every_status_returning_init_entry_point_keeps_the_error_contract(name):
    """As tests/test_capi_cpu.py: a refusal returns its code and leaves it as the last error; a success returns GSR_OK and
    leaves GSR_OK, directly after another entry point was refused; neither leaves a HIP text."""
    L = _capi.lib()
    refused, code, fine = INIT_ERROR_CONTRACT[name]
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert getattr(L, name)(*refused) == code
    assert L.gsr_last_error() == code and L.gsr_last_hip_error() == b""
    assert L.gsr_forward(*_forward_nulls()) == _INVALID and L.gsr_last_error() == _INVALID
    assert getattr(L, name)(*fine) == _capi.GSR_OK
    assert L.gsr_last_error() == _capi.GSR_OK and L.gsr_last_hip_error() == b""


@pytest.mark.parametrize("args, code", [
    ((-1, _AT, _AT, _AT, None), _INVALID),                                  # n < 0
    ((5, None, _AT, _AT, None), _INVALID), ((5, _AT, None, _AT, None), _INVALID), ((5, _AT, _AT, None, None), _INVALID),
    ((5, _AT + 2, _AT, _AT, None), _INVALID), ((5, _AT, _AT + 1, _AT, None), _INVALID),       # not 4-byte aligned
    ((5, _AT, _AT, _AT + 8, None), _INVALID),                               # temp not 16-byte aligned
    ((0, _AT + 2, _AT, _AT, None), _INVALID),                               # (alignment is refused whatever n is)
    ((_capi.GSR_KNN_MAX_POINTS + 1, _AT, _AT, _AT, None), _capi.GSR_ERR_TOO_LARGE),
    ((1 << 40, _AT, _AT, _AT, None), _capi.GSR_ERR_TOO_LARGE),
])
def test_knn_refusals_come_before_any_hip_call(args, code):
    L = _capi.lib()
    assert L.gsr_knn_mean_dist2(*args) == code
    assert L.gsr_last_error() == code and L.gsr_last_hip_error() == b""


def test_knn_temp_bytes():
    L = _capi.lib()
    for n in (-1, -(1 << 40), _capi.GSR_KNN_MAX_POINTS + 1, 1 << 40):
        assert L.gsr_knn_temp_bytes(n) == 0, n
    sizes = [L.gsr_knn_temp_bytes(n) for n in (0, 1, 2, 63, 64, 65, BLOCK, BLOCK + 1, 1_000_000, 5_834_784, _capi.GSR_KNN_MAX_POINTS)]
    assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert 40 * 1_000_000 < sizes[8] < 48 * 1_000_000                       # (two key and two value arrays, the sorted points, boxes)


# ---- ply.read_points_ply ----
def _write_points(path, xyz, rgb, normals=False, colour=True, fmt="binary_little_endian", extra=False):
    n = xyz.shape[0]
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if extra:
        fields.insert(1, ("confidence", "<f8"))
    if colour:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.zeros(n, np.dtype(fields))
    rec["x"], rec["y"], rec["z"] = xyz.T
    if colour:
        rec["red"], rec["green"], rec["blue"] = rgb.T
    if normals:
        rec["nx"] = 7.0
    said = {"<f4": "float", "<f8": "double", "u1": "uchar"}
    header = f"ply\nformat {fmt} 1.0\ncomment made by a test\nelement vertex {n}\n"
    header += "".join(f"property {said[t]} {k}\n" for k, t in fields) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode())
        if fmt == "ascii":
            f.write("".join(" ".join(str(v) for v in row) + "\n" for row in rec.tolist()).encode())
        else:
            f.write(rec.tobytes())


def _cloud(n=37):
    rng = np.random.default_rng(3)
    return rng.normal(size=(n, 3)).astype(F), rng.integers(0, 256, (n, 3)).astype(np.uint8)


@pytest.mark.parametrize("normals, extra", [(True, False), (False, False), (True, True)])
def test_read_points_ply_finds_the_properties_by_name(tmp_path, normals, extra):
    from gsrast_amd import ply
    xyz, rgb = _cloud()
    path = str(tmp_path / "points3D.ply")
    _write_points(path, xyz, rgb, normals=normals, extra=extra)
    got_xyz, got_rgb = ply.read_points_ply(path)
    assert got_xyz.dtype == F and got_rgb.dtype == np.uint8
    assert got_xyz.tobytes() == xyz.tobytes() and got_rgb.tobytes() == rgb.tobytes()


def test_read_points_ply_refusals_name_what_is_missing(tmp_path):
    from gsrast_amd import ply
    xyz, rgb = _cloud()
    path = str(tmp_path / "p.ply")
    _write_points(path, xyz, rgb, colour=False)
    with pytest.raises(ValueError, match="red, green, blue"):
        ply.read_points_ply(path)
    _write_points(path, xyz, rgb, fmt="ascii")
    with pytest.raises(ValueError, match="ascii"):
        ply.read_points_ply(path)
    _write_points(path, xyz, rgb)
    whole = open(path, "rb").read()
    open(path, "wb").write(whole[:-10])
    with pytest.raises(ValueError, match="ends before 37"):
        ply.read_points_ply(path)
    open(path, "wb").write(whole.replace(b"property float y\n", b"property double y\n"))
    with pytest.raises(ValueError, match="y is not float"):
        ply.read_points_ply(path)
    open(path, "wb").write(b"not a ply\n")
    with pytest.raises(ValueError, match="not a .ply"):
        ply.read_points_ply(path)


# ---- the Python refusals: before anything is launched (none of these reaches the library) ----
def test_python_refusals():
    import torch
    from gsrast_amd import init
    from gsrast_amd.autograd import GaussianParams
    for bad, what in ((torch.zeros(5, 3, dtype=torch.float64), "float64"), (torch.zeros(5, 4), r"\(5, 4\)"),
                      (torch.zeros(15), r"\(15,\)"), (torch.zeros(5, 3), "cpu"), (np.zeros((5, 3), F), "ndarray")):
        with pytest.raises(ValueError, match=what):
            init.knn_mean_dist2(bad)
        with pytest.raises(ValueError, match=what):
            init.initial_values(bad, torch.zeros(5, 3))
    with pytest.raises(ValueError, match=r"rgb is \(4, 3, 1\)"):
        GaussianParams.from_points(np.zeros((4, 3), F), np.zeros((4, 3, 1), F), device="cpu")
    with pytest.raises(ValueError, match="4 positions and 5 colours"):
        GaussianParams.from_points(np.zeros((4, 3), F), np.zeros((5, 3), F), device="cpu")
    xyz = np.zeros((4, 3), F)
    xyz[2, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        GaussianParams.from_points(xyz, np.zeros((4, 3), np.uint8), device="cpu")
