"""CPU: the depth channel's ABI (gsr_forward_args.out_depth, gsr_backward_args.dL_dout_depth / dL_ddepths / depth_sums_f64,
GSR_FLAG_DEPTH_INVERSE) and the float64 reference the GPU depth tests use (tests/test_gpu_depth*.py import it from here)."""
import ctypes as C
import os
import subprocess

import numpy as np

from gsrast_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference ------------------------------------------------------------------------------------------------------
def depth_values_f32(means3D, view, inverse=False):
    """d_i in float32 in the header's operation order: z = (V[2] x + V[6] y) + (V[10] z3 + V[14] 1), or 1 / z."""
    m = np.asarray(means3D, np.float32)
    v = np.asarray(view, np.float32).reshape(16)
    one = np.float32(1.0)
    z = (v[2] * m[:, 0] + v[6] * m[:, 1]) + (v[10] * m[:, 2] + v[14] * one)
    return (one / z).astype(np.float32) if inverse else z.astype(np.float32)


def depth_values_f64(mean3, view, inverse=False):
    v = np.asarray(view, np.float64).reshape(16)
    m = np.asarray(mean3, np.float64)
    z = v[2] * m[..., 0] + v[6] * m[..., 1] + v[10] * m[..., 2] + v[14]
    return 1.0 / z if inverse else z


def depth_mean_term(mean3, view, dL_dd, inverse=False):
    """What d_i adds to dL_dmeans3D: dL/dd_i (V[2], V[6], V[10]), times -1 / z^2 for inverse depth. mean3 [n,3], dL_dd [n]."""
    v = np.asarray(view, np.float64).reshape(16)
    g = np.asarray(dL_dd, np.float64)
    if inverse:
        z = depth_values_f64(mean3, view, False)
        g = -g / (z * z)
    return g[:, None] * np.array([v[2], v[6], v[10]])[None, :]


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _compile_and_run(tmp_path, body):
    src = tmp_path / "depth_abi.c"
    exe = tmp_path / "depth_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    return dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())


def test_depth_fields_match_the_header(tmp_path):
    fields = {"gsr_forward_args": (_capi.ForwardArgs, ["out_depth", "receipt", "plan_used"]),
              "gsr_backward_args": (_capi.BackwardArgs, ["dL_dout_depth", "dL_ddepths", "depth_sums_f64", "receipt"])}
    body = ""
    for cname, (_, names) in fields.items():
        body += f'printf("{cname} %zu\\n", sizeof({cname}));'
        body += "".join(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in names)
    body += 'printf("flag %u\\n", (unsigned)GSR_FLAG_DEPTH_INVERSE);'
    got = _compile_and_run(tmp_path, body)
    for cname, (cls, names) in fields.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f in names:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    # appended: the new fields are the last ones, behind everything an existing caller sets
    assert _capi.ForwardArgs._fields_[-1][0] == "out_depth"
    assert [f for f, _ in _capi.BackwardArgs._fields_[-3:]] == ["dL_dout_depth", "dL_ddepths", "depth_sums_f64"]
    assert int(got["flag"]) == 0x2000


def test_depth_flag_is_free():
    assert _capi.GSR_FLAG_DEPTH_INVERSE == 0x2000
    flags = [v for k, v in vars(_capi).items() if k.startswith("GSR_FLAG_") and k != "GSR_FLAG_DEPTH_INVERSE"]
    assert all(f & 0x2000 == 0 for f in flags)


def test_forward_struct_of_the_old_size_is_refused():
    L = _capi.lib()
    a = _capi.ForwardArgs()
    a.struct_size = _capi.ForwardArgs.out_depth.offset          # what a caller compiled against the header before sets
    assert L.gsr_forward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    b = _capi.BackwardArgs()
    b.struct_size = _capi.BackwardArgs.dL_dout_depth.offset
    assert L.gsr_backward(C.byref(b)) == _capi.GSR_ERR_INVALID_ARG


# ---- the reference against finite differences ---------------------------------------------------------------------------
def _tiny_view():
    from gsrast_amd import camera
    return np.asarray(camera.default_camera(32, 24, near=0.05, far=50.0, position=(0.3, -0.2, -4.0)).view, np.float64)


def test_depth_reference_against_finite_differences():
    """dL_dmeans3D through z (and 1 / z) of the reference, against central differences of d_i itself, both modes; and the
    float32 value in the pinned order against float64."""
    rng = np.random.default_rng(5)
    view = _tiny_view()
    means = rng.uniform(-1.0, 1.0, size=(6, 3))
    g = rng.normal(size=6)
    for inverse in (False, True):
        z = depth_values_f64(means, view, False)
        assert (z > 0).all()                                  # in front of the camera: positive
        exp = depth_mean_term(means, view, g, inverse)
        eps = 1e-6
        for j in range(3):
            dp, dm = means.copy(), means.copy()
            dp[:, j] += eps
            dm[:, j] -= eps
            fd = g * (depth_values_f64(dp, view, inverse) - depth_values_f64(dm, view, inverse)) / (2 * eps)
            assert np.allclose(exp[:, j], fd, rtol=1e-6, atol=1e-9), (inverse, j)
        m4 = np.concatenate([means, np.ones((6, 1))], 1).astype(np.float32)
        d32 = depth_values_f32(m4, view.astype(np.float32), inverse)
        assert d32.dtype == np.float32
        assert np.allclose(d32, depth_values_f64(means.astype(np.float32), view.astype(np.float32), inverse), rtol=1e-6)


def test_depth_blend_reference_is_a_colour_channel():
    """The per-pixel definition: sum d_i alpha_i T_i = channel 0 of the blend of colours (d, d, d) over a zero background,
    and its gradient w.r.t. d_i is that colour's (oracle/backward_np.py), checked by finite differences on a tiny frame."""
    from oracle import backward_np as B
    rng = np.random.default_rng(3)
    n, w, h = 5, 16, 16
    means2D = rng.uniform(2, 14, size=(n, 2))
    co = np.zeros((n, 4))
    co[:, 0] = co[:, 2] = rng.uniform(0.05, 0.2, size=n)
    co[:, 1] = rng.uniform(-0.02, 0.02, size=n)
    co[:, 3] = rng.uniform(0.3, 0.8, size=n)
    d = rng.uniform(1.0, 5.0, size=n)
    ranges = np.array([[0, n]])
    plist = np.arange(n)
    gd = rng.normal(size=(h, w))

    def frame(dd):
        out, ft, nc = B.blend_forward(means2D, co, np.repeat(dd[:, None], 3, 1), ranges, plist, w, h, (0.0, 0.0, 0.0))
        return out[0], ft, nc
    depth, ft, nc = frame(d)
    g3 = np.zeros((3, h, w))
    g3[0] = gd
    res = B.blend_backward(means2D, co, np.stack([d, 0 * d, 0 * d], 1), ranges, plist, nc, ft, w, h, (0.0, 0.0, 0.0), g3)
    for i in range(n):
        dp, dm = d.copy(), d.copy()
        dp[i] += 1e-6
        dm[i] -= 1e-6
        fd = float((gd * (frame(dp)[0] - frame(dm)[0])).sum()) / 2e-6
        assert abs(res["dL_dcolor"][i, 0] - fd) <= 1e-6 * max(1.0, abs(fd)), i
