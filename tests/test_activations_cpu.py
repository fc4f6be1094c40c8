"""CPU: the float64 reference of the activation backward (tests/activation_ref.py) against central differences; the two
entry points of csrc/activations.hip refuse incomplete arguments before they touch a device; GaussianParams.save_ply
writes the raw values bit for bit in the file's order."""
import ctypes as C

import numpy as np
import pytest

import activation_ref as A


def _raw(n, seed):
    """Logits and log-scales in [-4, 4], quaternions of norm in [0.3, 3]."""
    rng = np.random.default_rng(seed)
    xyz = rng.normal(0, 2, (n, 3))
    x = rng.uniform(-4, 4, n)
    s = rng.uniform(-4, 4, (n, 3))
    r = rng.normal(size=(n, 4))
    r *= (rng.uniform(0.3, 3.0, (n, 1)) / np.linalg.norm(r, axis=1, keepdims=True))
    return xyz, x, s, r


def test_reference_backward_matches_central_differences():
    """L = sum(w . activations) over 32 Gaussians; dL/draw by central differences with h = 1e-5 in float64: the truncation
    error is h^2 / 6 of a third derivative (here of the order of the first: 2e-11 relative), the rounding error 1e-16 / h =
    1e-11 of L's terms. Bound: 1e-8 of each array's largest entry."""
    n = 32
    xyz, x, s, r = _raw(n, 5)
    assert 0.3 - 1e-9 <= np.linalg.norm(r, axis=1).min() and np.linalg.norm(r, axis=1).max() <= 3.0 + 1e-9
    rng = np.random.default_rng(6)
    w = [rng.normal(size=(n, 4)), rng.normal(size=(n, 4)), rng.normal(size=(n, 4)), rng.normal(size=n)]

    def loss(xyz, x, s, r):
        return sum(float((wi * a).sum()) for wi, a in zip(w, A.activations(xyz, x, s, r)))
    got = A.backward(x, s, r, w[0], w[1], w[2], w[3])
    args = [xyz, x, s, r]
    h = 1e-5
    for k, name in ((0, "xyz"), (1, "opacity_logit"), (2, "log_scale"), (3, "rotation")):
        fd = np.zeros_like(args[k])
        for idx in np.ndindex(*args[k].shape):
            hi, lo = [a.copy() for a in args], [a.copy() for a in args]
            hi[k][idx] += h
            lo[k][idx] -= h
            fd[idx] = (loss(*hi) - loss(*lo)) / (2 * h)
        assert np.abs(fd).max() > 0.1, name
        err = np.abs(got[k] - fd).max()
        assert err <= 1e-8 * np.abs(fd).max(), (name, err)
    # the quaternion's gradient has no component along the quaternion (the activation does not depend on its length)
    assert np.abs((got[3] * r).sum(1)).max() <= 1e-14 * np.abs(got[3]).max() * 3.0
    # culled rows
    radii = np.ones(n, np.int32)
    radii[::3] = 0
    radii[1] = -1
    cut = A.backward(x, s, r, w[0], w[1], w[2], w[3], radii)
    for a, b in zip(cut, got):
        assert (a[radii <= 0] == 0).all() and (a[radii > 0] == b[radii > 0]).all()


P = 0x10000          # a non-null, 16-byte aligned address that is never dereferenced: these calls return before any launch


def test_activate_params_refuses_missing_pointers():
    from gsrast_amd import _capi
    L = _capi.lib()
    assert L.gsr_activate_params(0, *([None] * 8), None) == _capi.GSR_OK
    assert L.gsr_activate_params(-3, *([None] * 8), None) == _capi.GSR_OK
    for missing in range(8):
        ptrs = [P] * 8
        ptrs[missing] = None
        assert L.gsr_activate_params(5, *ptrs, None) == _capi.GSR_ERR_INVALID_ARG, missing
    for odd in (0, 2, 3, 4, 5, 6):                      # the arrays moved in 16-byte vectors
        ptrs = [P] * 8
        ptrs[odd] = P + 4
        assert L.gsr_activate_params(5, *ptrs, None) == _capi.GSR_ERR_INVALID_ARG, odd


def test_activate_params_backward_refuses_missing_pointers():
    from gsrast_amd import _capi
    L = _capi.lib()
    call = L.gsr_activate_params_backward
    # arguments: raw_opacity, raw_scales, raw_rotations, radii, g_means, g_scales, g_rotations, g_conic_opacity,
    #            out_means, out_opacity, out_scales, out_rotations
    assert call(0, *([None] * 12), None) == _capi.GSR_OK
    assert call(7, *([None] * 12), None) == _capi.GSR_OK          # no output asked for: nothing to do
    needs = {8: (4,), 9: (0, 7), 10: (1, 5), 11: (2, 6)}           # output -> the inputs it is computed from
    for out, ins in needs.items():
        for missing in ins:
            ptrs = [None] * 12
            ptrs[out] = P
            for i in ins:
                ptrs[i] = P
            ptrs[missing] = None
            assert call(7, *ptrs, None) == _capi.GSR_ERR_INVALID_ARG, (out, missing)
    for out, ins in needs.items():
        if out == 9:
            continue                                               # (one float per Gaussian: any alignment)
        ptrs = [None] * 12
        for i in ins:
            ptrs[i] = P
        ptrs[out] = P + 8
        assert call(7, *ptrs, None) == _capi.GSR_ERR_INVALID_ARG, out


@pytest.mark.parametrize("layout", ["file", "coefficient_major"])
def test_save_ply_writes_every_raw_value_bit_for_bit(tmp_path, layout):
    from gsrast_amd import ply
    from gsrast_amd.autograd import GaussianParams
    n = 37
    rng = np.random.default_rng(11)
    xyz, x, s, r = (a.astype(np.float32) for a in _raw(n, 12))
    shs = rng.normal(size=(n, 48)).astype(np.float32)
    xyz[0, 0], x[1], s[2, 1], r[3, 2], shs[4, 17] = -0.0, 90.0, -100.0, 1e-40, 3.0e38      # signed zero, extremes, a denormal
    p = GaussianParams.from_raw(xyz, x, s, r, shs, sh_layout=layout, device="cpu")
    path = str(tmp_path / "scene.ply")
    p.save_ply(path)
    cnt, off = ply.parse_header(path)
    assert cnt == n
    rec = np.fromfile(path, dtype="<f4", offset=off).reshape(n, ply.RECORD_FLOATS)
    want_sh = shs.copy()
    if layout == "coefficient_major":                   # shs[3 k + ch] is f_rest[15 ch + (k - 1)] of the file, k = 1..15
        for k in range(1, 16):
            for ch in range(3):
                want_sh[:, 3 + 15 * ch + (k - 1)] = shs[:, 3 * k + ch]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert (bits(rec[:, 0:3]) == bits(xyz)).all() and (rec[:, 3:6] == 0).all()
    assert (bits(rec[:, 6:54]) == bits(want_sh)).all()
    assert (bits(rec[:, 54]) == bits(x)).all() and (bits(rec[:, 55:58]) == bits(s)).all()
    assert (bits(rec[:, 58:62]) == bits(r)).all()
    # ... and from_ply gives the same parameters back, in the layout asked for
    q = GaussianParams.from_ply(path, sh_layout=layout, device="cpu")
    for a, b in zip(p.parameters(), q.parameters()):
        assert (bits(a.detach().numpy()) == bits(b.detach().numpy())).all()
