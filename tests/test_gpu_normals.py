"""GPU: the two operators of the normal-consistency loss (include/gsrast_amd_normals.h, gsrast_amd/normals.py,
rasterize / render(..., normals=True)). The four calls against tests/normals_ref.py — the forwards bit for bit against the
float32 restatements, the backwards against the float64 autograd functions within one float32 ulp (the project's standing bound
for chains evaluated in double, tests/test_gpu_filter3d.py) — and the composition with the library: the normal map's bits, the
tuple's order, the default path untouched, the rotations' gradient through the normals, the refusals, a short training run.
The references' own preconditions are tests/test_normals_cpu.py's."""
import ctypes as C

import numpy as np
import pytest

import normals_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 64                        # floats of sentinel on each side of every array written
SIZES = [1, 63, 64, 65, 255, 256, 257, 1000]
# the issue's shapes, and the edges of the kernels' 64 x 4 workgroup, +-1
SHAPES = [(1, 1), (2, 7), (3, 3), (3, 65), (65, 3), (17, 33), (64, 48), (67, 131), (4, 64), (5, 65), (3, 63), (8, 128), (9, 129)]
FLAGS = {"gscuda": 0, "inria": 0x4}


def _torch():
    import torch
    return torch


def _capi():
    from gsrast_amd import _capi
    return _capi


def _dev(a, dtype=np.float32):
    return _torch().from_numpy(np.array(a, dtype)).cuda()


def _bits(t):
    torch = _torch()
    t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t))
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


class _Guarded:
    """A device array of `floats` floats between two runs of 0xFF bytes."""

    def __init__(self, floats):
        torch = _torch()
        self.buf = torch.full((4 * (floats + 2 * PAD),), 0xFF, dtype=torch.uint8, device="cuda")
        self.floats = floats

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def inner(self):
        return self.buf[4 * PAD:4 * (PAD + self.floats)].view(_torch().float32)

    def intact(self):
        return bool((self.buf[:4 * PAD] == 0xFF).all()) and bool((self.buf[4 * (PAD + self.floats):] == 0xFF).all())


def _stream(stream):
    return stream if stream is not None else _torch().cuda.current_stream().cuda_stream


def _gaussian_forward(means, scales, quats, view, semantics, stream=None):
    capi, n = _capi(), int(means.shape[0])
    out = _Guarded(3 * n)
    a = capi.GaussianNormalsArgs()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), FLAGS[semantics], n
    a.means3D, a.scales, a.rotations, a.view_matrix = means.data_ptr(), scales.data_ptr(), quats.data_ptr(), view.data_ptr()
    a.normals, a.stream = out.ptr, _stream(stream)
    _torch().cuda.synchronize()
    capi.call("gsr_gaussian_normals_forward", C.byref(a))
    _torch().cuda.synchronize()
    assert out.intact(), "a write outside normals"
    return out.inner().reshape(n, 3)


def _gaussian_backward(means, scales, quats, view, g, radii, semantics):
    capi, n = _capi(), int(means.shape[0])
    out = _Guarded(4 * n)
    a = capi.GaussianNormalsBackwardArgs()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), FLAGS[semantics], n
    a.means3D, a.scales, a.rotations, a.view_matrix = means.data_ptr(), scales.data_ptr(), quats.data_ptr(), view.data_ptr()
    a.dL_dnormals, a.radii = g.data_ptr(), (radii.data_ptr() if radii is not None else None)
    a.dL_drotations, a.stream = out.ptr, _stream(None)
    _torch().cuda.synchronize()
    capi.call("gsr_gaussian_normals_backward", C.byref(a))
    _torch().cuda.synchronize()
    assert out.intact(), "a write outside dL_drotations"
    return out.inner().reshape(n, 4)


def _depth_forward(depth, tan_fov, semantics, stream=None):
    capi = _capi()
    h, w = (int(v) for v in depth.shape)
    out = _Guarded(3 * h * w)
    a = capi.DepthNormalsArgs()
    a.struct_size, a.flags, a.width, a.height = C.sizeof(a), FLAGS[semantics], w, h
    a.tan_fovx, a.tan_fovy = tan_fov
    a.depth, a.normals, a.stream = depth.data_ptr(), out.ptr, _stream(stream)
    _torch().cuda.synchronize()
    capi.call("gsr_depth_normals_forward", C.byref(a))
    _torch().cuda.synchronize()
    assert out.intact(), "a write outside normals"
    return out.inner().reshape(3, h, w)


def _depth_backward(depth, g, tan_fov, semantics):
    capi = _capi()
    h, w = (int(v) for v in depth.shape)
    out = _Guarded(h * w)
    a = capi.DepthNormalsBackwardArgs()
    a.struct_size, a.flags, a.width, a.height = C.sizeof(a), FLAGS[semantics], w, h
    a.tan_fovx, a.tan_fovy = tan_fov
    a.depth, a.dL_dnormals, a.dL_ddepth, a.stream = depth.data_ptr(), g.data_ptr(), out.ptr, _stream(None)
    _torch().cuda.synchronize()
    capi.call("gsr_depth_normals_backward", C.byref(a))
    _torch().cuda.synchronize()
    assert out.intact(), "a write outside dL_ddepth"
    return out.inner().reshape(h, w)


def _view(semantics):
    return R.random_view(3, mirrored=(semantics == "gscuda"))


# ---- Gaussian normals, forward --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", R.PROFILES)
@pytest.mark.parametrize("n", SIZES)
def test_gaussian_normals_are_the_restatement_bit_for_bit(n, semantics):
    """N around the wave and the workgroup; the case's first rows hold ties, zeros, 1e9 and NaN scales, a zero, a NaN, an
    unnormalised and a tiny quaternion; a tenth of the means lie behind the camera."""
    torch = _torch()
    means, scales, quats = R.gaussian_case(n, seed=0)
    view = _view(semantics)
    want, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    dev = [_dev(v) for v in (means, scales, quats, view)]
    got = _gaussian_forward(*dev, semantics)
    assert _same_bits(got, want), (n, np.nonzero((_bits(got) != _bits(want)).any(1))[0][:8])
    assert (_bits(got)[~dec["valid"]] == 0).all()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert _same_bits(_gaussian_forward(*dev, semantics, stream=side.cuda_stream), want)
    assert all(_same_bits(t, v) for t, v in zip(dev, (means, scales, quats, view))), "an input was written"
    if n == 1000:
        from gsrast_amd import normals
        assert _same_bits(normals.gaussian_normals(*dev, semantics=semantics), want)
        with pytest.raises(ValueError):
            normals.gaussian_normals(*dev[:3], dev[3].clone().requires_grad_(True), semantics=semantics)
        with pytest.raises(ValueError):
            normals.gaussian_normals(*dev, semantics="opengl")


# ---- Gaussian normals, backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", R.PROFILES)
def test_gaussian_normals_backward_is_the_float64_function_rounded_once(semantics):
    n = 1000
    rng = np.random.default_rng(31)
    means, scales, quats = (a.copy() for a in R.gaussian_case(n, seed=21, edges=False))
    view = _view(semantics)
    g = R.seed_gradient((n, 3), seed=8)
    radii = rng.integers(1, 40, n).astype(np.int32)
    off = rng.uniform(size=n) < 1.0 / 6.0
    radii[off] = np.where(rng.uniform(size=off.sum()) < 0.5, 0, -1)
    nograd = ~off & (rng.uniform(size=n) < 0.1)
    g[nograd] = 0.0
    g[np.nonzero(nograd)[0][:3], 1] = -0.0
    poisoned = np.concatenate([np.nonzero(off)[0][:5], np.nonzero(nograd)[0][:5]])
    quats[poisoned] = np.nan
    means[poisoned[::2]] = np.nan
    scales[poisoned[1::2]] = np.nan
    g[np.nonzero(off)[0][:3]] = np.nan
    _, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    live = ~off & ~nograd
    assert dec["valid"][live].all() and live.sum() >= 600
    dev = [_dev(v) for v in (means, scales, quats, view, g)]
    before = [t.clone() for t in dev]
    rd = _dev(radii, np.int32)
    got = _gaussian_backward(*dev, rd, semantics).cpu().numpy()
    assert (got[~live].view(np.uint32) == 0).all(), "culled and zero-gradient rows are +0 bit for bit"
    ref = R.gaussian_gradients64(np.nan_to_num(quats), view, np.nan_to_num(g), dec, semantics)
    want = ref[live].astype(F)
    err = np.abs(got[live].astype(np.float64) - want.astype(np.float64))
    worst = float((err / R.ulp32(want)).max())
    print(f"[normals] {semantics} dL_drotations: worst error {worst:.2f} ulp of the float64 value rounded to float32")
    assert np.isfinite(got).all() and (err <= R.ulp32(want)).all(), worst
    assert (np.abs(want).max(1) > 0).all()
    again = _gaussian_backward(*dev, rd, semantics)
    assert _same_bits(again, got)
    # radii == NULL: every row with a gradient is computed; the rows that had a tile are the same bits
    free = _gaussian_backward(*dev, None, semantics).cpu().numpy()
    assert np.array_equal(free[live].view(np.uint32), got[live].view(np.uint32))
    finite_off = off & np.isfinite(quats).all(1) & np.isfinite(g).all(1) & np.isfinite(means).all(1) & np.isfinite(scales).all(1)
    assert finite_off.sum() >= 50 and (free[finite_off] != 0).any(1).all()
    assert all(_same_bits(b, t) for b, t in zip(before, dev)), "an input was written"
    # rows whose forward wrote zeros get no gradient
    means, scales, quats = R.gaussian_case(64, seed=0)
    _, dec = R.gaussian_normals_f32(means, scales, quats, view, semantics)
    assert (~dec["valid"]).any()
    got = _gaussian_backward(_dev(means), _dev(scales), _dev(quats), dev[3], _dev(np.ones((64, 3), F)), None, semantics).cpu().numpy()
    assert (got[~dec["valid"]].view(np.uint32) == 0).all() and np.isfinite(got).all()


# ---- depth normals, forward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", R.PROFILES)
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_normals_are_the_restatement_bit_for_bit(shape, semantics):
    """Images with holes (0, -1, +-inf, NaN), a constant plane, and a tilted plane, at every shape."""
    h, w = shape
    normal = np.array([0.3, -0.2, -1.0]) / np.linalg.norm([0.3, -0.2, -1.0])
    plane = R.plane_depth(h, w, normal, -4.0, R.TAN_FOV, semantics).astype(F)
    for name, depth in (("holes", R.depth_case(h, w, seed=1)), ("constant", np.full((h, w), 2.5, F)), ("plane", plane)):
        want, dec = R.depth_normals_f32(depth, R.TAN_FOV, semantics)
        d = _dev(depth)
        got = _depth_forward(d, R.TAN_FOV, semantics)
        assert _same_bits(got, want), (name, shape, int((_bits(got) != _bits(want)).sum()))
        assert _same_bits(d, depth), "the input was written"
        if name == "constant" and h >= 3 and w >= 3:
            inner = got[:, 1:-1, 1:-1].cpu().numpy()
            assert (inner[0] == 0).all() and (inner[1] == 0).all() and (inner[2] == -1).all()
            edge = np.ones((h, w), bool)
            edge[1:-1, 1:-1] = False
            assert (_bits(got)[:, edge] == 0).all()
        if name == "plane" and h >= 3 and w >= 3:
            # (tests/test_normals_cpu.py: the float64 function of these rounded depths is within 6e-5 of the plane's normal on
            # 33 x 65; the float32 restatement adds its own roundings of the same size: 2e-4 at these baselines)
            import torch
            t = torch.from_numpy(depth.astype(np.float64))
            n64 = R.depth_normals64(t, t, t, t, R.TAN_FOV, semantics, dec).numpy()
            assert dec["valid"][1:-1, 1:-1].all() and np.abs(got.cpu().numpy() - n64).max() <= 2e-4
            assert np.abs(n64[:, 1:-1, 1:-1] - normal[:, None, None]).max() <= 2e-4
    if shape == (67, 131):
        torch = _torch()
        from gsrast_amd import normals
        depth = R.depth_case(h, w, seed=1)
        want, _ = R.depth_normals_f32(depth, R.TAN_FOV, semantics)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        assert _same_bits(_depth_forward(_dev(depth), R.TAN_FOV, semantics, stream=side.cuda_stream), want)
        assert _same_bits(normals.depth_normals(_dev(depth), R.TAN_FOV, semantics=semantics), want)
        with pytest.raises(ValueError):
            normals.depth_normals(_dev(depth)[None], R.TAN_FOV, semantics=semantics)


# ---- depth normals, backward --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", R.PROFILES)
@pytest.mark.parametrize("shape", SHAPES)
def test_depth_normals_backward_is_the_float64_gather_rounded_once(shape, semantics):
    """Where |want| >= 2^-20 sum |terms|: within one float32 ulp of the float64 sum rounded to float32; elsewhere within
    ulp32(2^-20 sum |terms|) — double carries 29 more bits than float32, so 20 bits of cancellation still leave the rounding the
    only error. At most 1 % of the pixels may fall in the second branch."""
    h, w = shape
    depth = R.depth_case(h, w, seed=1)
    g = R.seed_gradient((3, h, w), seed=h)
    _, dec = R.depth_normals_f32(depth, R.TAN_FOV, semantics)
    total, terms = R.depth_gradients64(depth, g, R.TAN_FOV, semantics, dec)
    d, gd = _dev(depth), _dev(g)
    got_t = _depth_backward(d, gd, R.TAN_FOV, semantics)
    got = got_t.cpu().numpy()
    assert np.isfinite(got).all()
    mass = np.abs(terms).sum(0)
    want = total.astype(F)
    tight = np.abs(total) >= 2.0 ** -20 * mass
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    loose = ~tight
    assert loose.sum() <= 0.01 * h * w or h * w < 100 and loose.sum() <= 1
    if tight.any() and mass.max() > 0:
        on = tight & (mass > 0)
        worst = float((err[on] / R.ulp32(want[on])).max()) if on.any() else 0.0
        print(f"[normals] {semantics} {h} x {w} dL_ddepth: worst error {worst:.2f} ulp; {int(loose.sum())} pixels under the cancellation bound")
    assert (err[tight] <= R.ulp32(want[tight])).all()
    assert (err[loose] <= R.ulp32(2.0 ** -20 * mass[loose])).all()
    # pixels without a valid neighbour: +0; pixels next to holes: the gradient of their valid neighbours only (the terms say so)
    assert (got[mass == 0].view(np.uint32) == 0).all()
    if h >= 17:
        ok = dec["valid"]
        partial = np.zeros((h, w), bool)
        partial[1:-1, 1:-1] = (ok[:-2, 1:-1].astype(int) + ok[2:, 1:-1] + ok[1:-1, :-2] + ok[1:-1, 2:]) < 4
        partial &= mass > 0
        assert partial.sum() >= 10 and (got[partial] != 0).all()
    assert _same_bits(_depth_backward(d, gd, R.TAN_FOV, semantics), got_t), "two calls differ"
    assert _same_bits(d, depth) and _same_bits(gd, g), "an input was written"
    if shape == (64, 48):
        torch = _torch()
        from gsrast_amd import normals
        leaf = _dev(depth).requires_grad_(True)
        (normals.depth_normals(leaf, R.TAN_FOV, semantics=semantics) * gd).sum().backward()
        assert _same_bits(leaf.grad, got_t)


# ---- through the library ------------------------------------------------------------------------------------------------------------------
def _helpers():
    import test_gpu_autograd as T
    return T


def _leaves(profile, requires=True):
    """The activated arrays of tests/test_gpu_autograd.py's scene as leaves, its shs, and the camera's tensors."""
    torch = _torch()
    from gsrast_amd import autograd
    T = _helpers()
    params = T._params(profile)
    with torch.no_grad():
        act = autograd.activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
    leaves = [t.clone().requires_grad_(requires) for t in act]
    return leaves, params.shs.detach().clone()


@pytest.mark.parametrize("profile", R.PROFILES)
def test_normal_map_is_the_feature_map_of_the_gaussian_normals_and_the_tuple_order_holds(profile):
    torch = _torch()
    from gsrast_amd import autograd, normals
    import features_ref as FR
    T = _helpers()
    cam = T._cam(1)
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, torch.device("cuda:0"))
    leaves, shs = _leaves(profile, requires=False)
    n = int(leaves[0].shape[0])
    kw = dict(**T._kw(profile), **T.DRAW)
    call = lambda rast, **more: autograd.rasterize(rast, *leaves, shs, view, proj, cam_pos, (tx, ty), **kw, **more)
    rast = T._rasterizer()
    plain = call(rast)
    per_gaussian = normals.gaussian_normals(leaves[0], leaves[1], leaves[2], view, semantics=profile)
    want_map = rast.render_features(per_gaussian)
    assert float(want_map.abs().max()) > 0.1
    out = call(T._rasterizer(), normals=True)
    assert len(plain) == 3 and len(out) == 4 and out[1] is None and tuple(out[3].shape) == (3, T.H, T.W)
    assert all(_same_bits(a, b) for a, b in zip((plain[0], plain[2]), (out[0], out[2]))) and _same_bits(out[3], want_map)
    # with features of C = 1 and C = 253: both maps are the separate calls' bits; C = 254 raises
    for c in (1, 253):
        feats = _dev(FR.features_of(n, c))
        rast = T._rasterizer()
        out = call(rast, features=feats, normals=True)
        assert len(out) == 5 and tuple(out[3].shape) == (c, T.H, T.W) and tuple(out[4].shape) == (3, T.H, T.W)
        assert _same_bits(out[4], want_map) and _same_bits(out[3], rast.render_features(feats))
    with pytest.raises(ValueError, match="channels"):
        call(T._rasterizer(), features=_dev(FR.features_of(n, 254)), normals=True)
    # the order with and without depth, features and distortion: (color, depth, opacity[, features][, normals][, distortion])
    feats = _dev(FR.features_of(n, 2))
    for depth in (False, True):
        for with_f in (False, True):
            for with_d in (False, True):
                more = dict(depth=depth, **({"features": feats} if with_f else {}), **({"distortion": "depth"} if with_d else {}))
                base, out = call(T._rasterizer(), **more), call(T._rasterizer(), normals=True, **more)
                at = 3 + int(with_f)
                assert len(out) == len(base) + 1 == 4 + int(with_f) + int(with_d), more
                assert (out[1] is None) == (not depth) and _same_bits(out[at], want_map), more
                rest = out[:at] + out[at + 1:]
                assert all((a is None and b is None) or _same_bits(a, b) for a, b in zip(base, rest)), more
    # a view that requires a gradient is refused
    with pytest.raises(ValueError, match="view requires a gradient"):
        autograd.rasterize(T._rasterizer(), *leaves, shs, view.clone().requires_grad_(True), proj, cam_pos, (tx, ty), normals=True, **kw)


@pytest.mark.parametrize("profile", R.PROFILES)
def test_render_without_normals_is_what_it_was_and_a_stale_graph_is_refused(profile):
    torch = _torch()
    from gsrast_amd import autograd, normals
    T = _helpers()
    cam = T._cam(1)
    wt, wdt, _, _ = T._weights()
    runs = []
    for extra in ({}, {"normals": False}, {"normals": True}):
        params, rast = T._params(profile), T._rasterizer()
        out = autograd.render(params, rast, cam, depth=True, **T._kw(profile), **T.DRAW, **extra)
        assert len(out) == (4 if extra.get("normals") else 3)
        ((wt * out[0]).sum() + (wdt * out[1]).sum()).backward()
        runs.append(list(out[:3]) + [getattr(params, k).grad for k in T.RAW])
    # (a loss that does not use the normal map: the same bits with the option too)
    assert all(_same_bits(a, b) for a, b in zip(runs[0], runs[1])) and all(_same_bits(a, b) for a, b in zip(runs[0], runs[2]))
    params, rast = T._params(profile), T._rasterizer()
    nmap = autograd.render(params, rast, cam, normals=True, **T._kw(profile), **T.DRAW)[3]
    autograd.render(params, rast, T._cam(2), **T._kw(profile), **T.DRAW)
    with pytest.raises(RuntimeError, match="has drawn another frame"):
        nmap.sum().backward()
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, rast.device)
    with pytest.raises(ValueError, match="view requires a gradient"):
        autograd.render(T._params(profile), T._rasterizer(), (view.clone().requires_grad_(True), proj, cam_pos, tx, ty), normals=True,
                        **T._kw(profile), **T.DRAW)


@pytest.mark.parametrize("variant", ["plain", "antialiased and filtered"])
@pytest.mark.parametrize("profile", R.PROFILES)
def test_rotation_gradient_of_the_consistency_loss_through_the_normals(profile, variant):
    """Three graphs of the same frame and the same loss, normal_consistency(...).mean():
      A  render(normals=True) of the raw parameters;
      B  rasterize(normals=True) of the activated (and smoothed) arrays as leaves;
      C  rasterize(features=F) of the same leaves, F the per-Gaussian normals as a leaf: everything but the path through them.
    The maps of all three are the same bits. B's and C's rotation gradients differ by exactly the path through the normals, and
    that difference is held against the float64 composition — tests/features_ref.py's walk for dL_dfeatures, tests/normals_ref.py's
    chain from there to the rotation — within the feature backward's own bound taken through the chain (|J| bound, J the normals'
    Jacobian), plus what float32 adds where autograd sums the two paths and both graphs round their results: 4 x 2^-24 of the two
    gradients' magnitudes. A's raw gradient is B's taken through tests/activation_ref.py, within two float32 roundings of a chain
    evaluated in double (4 x 2^-24 of the largest entry, as tests/test_gpu_filter3d.py holds its composition)."""
    torch = _torch()
    from gsrast_amd import autograd, filter3d, normals
    import activation_ref as A
    import features_ref as FR
    from test_gpu_features import _state
    T = _helpers()
    cam = T._cam(1)
    tan = (float(cam.tan_fovx), float(cam.tan_fovy))
    raw = T._raw_scene(profile)
    n = len(raw["xyz"])
    aa = variant != "plain"
    filt = torch.full((n,), 0.05, dtype=torch.float32, device="cuda") if aa else None
    kw = dict(depth=True, opacity_grad=True, antialiased=aa, **T._kw(profile), **T.DRAW)
    loss_of = lambda nmap, dmap, omap: normals.normal_consistency(nmap, dmap, omap, tan, semantics=profile).mean()
    # A
    params, slot = T._params(profile), autograd.RadiiSlot()
    maps_a = autograd.render(params, T._rasterizer(), cam, normals=True, radii_slot=slot, filter_3d=filt, **kw)
    loss = loss_of(maps_a[3], maps_a[1], maps_a[2])
    loss.backward()
    assert 0.0 < float(loss.detach()) < 2.0
    radii = slot.radii.cpu().numpy()
    seen = radii > 0
    # B
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, torch.device("cuda:0"))
    with torch.no_grad():
        act = list(autograd.activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation))
        if filt is not None:
            act[1], act[3] = filter3d.smoothed(act[1], act[3], filt)
    shs = params.shs.detach().clone()
    leaves = [t.clone().requires_grad_(True) for t in act]
    rast_b = T._rasterizer()
    maps_b = autograd.rasterize(rast_b, *leaves, shs, view, proj, cam_pos, (tx, ty), normals=True, **kw)
    assert all(_same_bits(a, b) for a, b in zip(maps_a, maps_b))
    maps_b[3].retain_grad()
    loss_of(maps_b[3], maps_b[1], maps_b[2]).backward()
    st = _state(rast_b)
    g_map = maps_b[3].grad.cpu().numpy()
    # C
    per_gaussian = normals.gaussian_normals(act[0], act[1], act[2], view, semantics=profile)
    want_n, dec = R.gaussian_normals_f32(act[0].cpu().numpy(), act[1].cpu().numpy(), act[2].cpu().numpy(), view.cpu().numpy(), profile)
    assert _same_bits(per_gaussian, want_n) and dec["valid"].all()
    leaf = per_gaussian.clone().requires_grad_(True)
    leaves_c = [t.clone().requires_grad_(True) for t in act]
    maps_c = autograd.rasterize(T._rasterizer(), *leaves_c, shs, view, proj, cam_pos, (tx, ty), features=leaf, **kw)
    assert all(_same_bits(a, b) for a, b in zip(maps_b, maps_c))
    loss_of(maps_c[3], maps_c[1], maps_c[2]).backward()
    for i, k in ((0, "means3D"), (1, "scales"), (3, "opacities")):          # nothing but the rotation hears of the normals
        a, b = leaves[i].grad.double(), leaves_c[i].grad.double()
        assert float((a - b).abs().max()) <= 2.0 ** -22 * float(b.abs().max()), k
    total, geom = leaves[2].grad.cpu().numpy().astype(np.float64), leaves_c[2].grad.cpu().numpy().astype(np.float64)
    # the float64 composition
    ref = FR.backward(st, want_n, None, g_map, T.W, T.H, FR.T_CUTOFF[profile])
    d_chan, b_chan = ref["d_chan"], FR.bound(ref, "d_chan")
    assert (np.abs(leaf.grad.cpu().numpy() - d_chan) <= b_chan).all()
    rot_act, view_np = act[2].cpu().numpy(), view.cpu().numpy()
    chain = lambda g: R.gaussian_gradients64(rot_act, view_np, g, dec, profile) * seen[:, None]
    want = chain(d_chan)
    bound = sum(np.abs(chain(np.eye(3)[c][None, :].repeat(n, 0))) * b_chan[:, c:c + 1] for c in range(3))
    bound = bound + 4.0 * 2.0 ** -24 * (np.abs(total).max(1, keepdims=True) + np.abs(geom).max(1, keepdims=True))
    err = np.abs((total - geom) - want)
    top = float(np.abs(want).max())
    print(f"[normals] {profile} {variant}: dL_drotations through the normals, largest entry {top:.3e} (of {float(np.abs(total).max()):.3e} in all), "
          f"worst error {float(err.max()):.3e}, worst error / bound {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert top > 10.0 * float(bound.max()), "the path through the normals is too faint on this scene to be checked"
    assert (total[~seen] == geom[~seen]).all()
    # A's raw gradient is B's through the activation
    want_raw = A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], np.zeros((n, 4)), np.zeros((n, 4)), total, np.zeros(n),
                          radii=radii)[3]
    got_raw = params.rotation.grad.cpu().numpy().astype(np.float64)
    assert float(np.abs(got_raw - want_raw).max()) <= 4.0 * 2.0 ** -24 * float(np.abs(want_raw).max()) and (got_raw[~seen] == 0).all()
    share = float(np.abs(A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], np.zeros((n, 4)), np.zeros((n, 4)), geom, np.zeros(n),
                                    radii=radii)[3] - want_raw).max()) / float(np.abs(want_raw).max())
    assert share > 1e-3, "a backward that dropped the normals' gradient would not show"


def test_five_training_steps_with_the_normal_term():
    """Flat splats (one scale a twelfth of the others) with the scene's seeded orientations: five Adam steps on the
    normal-consistency term alone lower it."""
    torch = _torch()
    from gsrast_amd import autograd, normals
    from gsrast_amd.optim import GaussianAdam
    T = _helpers()
    profile = "inria"
    cam, rast = T._cam(1), T._rasterizer()
    tan = (float(cam.tan_fovx), float(cam.tan_fovy))
    raw = {k: v.copy() for k, v in T._raw_scene(profile).items()}
    raw["log_scale"][:, 2] -= np.float32(np.log(12.0))
    params = autograd.GaussianParams.from_raw(*(raw[k] for k in T.RAW), sh_layout="coefficient_major", device="cuda:0")
    rates = {"xyz": 1e-3, "opacity_logit": 1e-2, "log_scale": 5e-3, "rotation": 2e-2, "shs": 1e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    slot, losses = autograd.RadiiSlot(), []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        color, dmap, omap, nmap, dist = autograd.render(params, rast, cam, depth=True, opacity_grad=True, normals=True, distortion="depth",
                                                        radii_slot=slot, **T._kw(profile))
        loss = normals.normal_consistency(nmap, dmap, omap, tan, semantics=profile).mean()
        losses.append(float(loss.detach()))
        loss.backward()
        for k in T.RAW[:4]:
            grad = getattr(params, k).grad
            assert bool(torch.isfinite(grad).all()) and bool((grad[slot.radii <= 0] == 0).all()), k
        assert bool((params.rotation.grad != 0).any())
        opt.step(slot.radii)
    print(f"[normals] normal-consistency loss over five steps: {' '.join(f'{v:.6f}' for v in losses)}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
