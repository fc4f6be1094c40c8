"""GPU: gsr_knn_mean_dist2 bit for bit against the brute force of tests/knn_ref.py — sentinels on both sides of everything
the call may write, xyz unchanged, two runs the same bits — over the sizes at which the search takes another path and the
scenes whose guards tests/test_knn_cpu.py checks; gsrast_amd.init against the same torch expressions on the reference; and
GaussianParams.from_points carried through one training step."""
import ctypes as C

import numpy as np
import pytest

from test_knn_cpu import SCENES, SIZES, reference_of, scene

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FC0BEEF                    # (as a float: a NaN, so that a sentinel read as a coordinate or a distance shows)
GAP = 64                                 # sentinel words on both sides of every array
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class _Arena:
    """One device buffer of 4-byte words filled with a sentinel; every array is a 16-byte-aligned slice of it with GAP
    sentinels on both sides (the pattern of tests/test_gpu_densify.py)."""

    def __init__(self, sizes):
        import torch
        self.slices, at = {}, GAP
        for name, count in sizes.items():
            self.slices[name] = slice(at, at + count)
            at += (count + 3) // 4 * 4 + GAP
        self.host = np.full(at, SENTINEL, np.uint32)
        self.dev = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0

    def put(self, name, a):
        import torch
        a = _bits(a).reshape(-1)
        assert a.size == self.slices[name].stop - self.slices[name].start, name
        self.host[self.slices[name]] = a
        self.dev[self.slices[name]] = torch.from_numpy(a.view(np.int32).copy()).cuda()

    def ptr(self, name):
        return self.dev.data_ptr() + 4 * self.slices[name].start

    def read(self):
        import torch
        torch.cuda.synchronize()
        return self.dev.cpu().numpy().view(np.uint32)

    def outside(self, got, names):
        """The words of `got` that belong to none of the arrays `names`, and what they must hold."""
        free = np.ones(got.size, bool)
        for name in names:
            free[self.slices[name]] = False
        return got[free], self.host[free]


def _run(xyz, runs=2):
    """gsr_knn_mean_dist2 on xyz, `runs` times with one temp into separate outputs -> the outputs' bits; asserts the
    sentinels, the untouched xyz and GSR_OK on the way."""
    from gsrast_amd import _capi
    L = _capi.lib()
    n = xyz.shape[0]
    temp_bytes = int(L.gsr_knn_temp_bytes(n))
    assert temp_bytes > 0 and temp_bytes % 16 == 0
    outs = [f"out{r}" for r in range(runs)]
    arena = _Arena({"xyz": 3 * n, **{o: n for o in outs}, "temp": temp_bytes // 4})
    arena.put("xyz", xyz)
    for o in outs:
        _capi.call("gsr_knn_mean_dist2", n, arena.ptr("xyz"), arena.ptr(o), arena.ptr("temp"), _capi.stream(arena.dev.device),
                   device=arena.dev.device)
    got = arena.read()
    rest, want = arena.outside(got, outs + ["temp"])                 # the sentinels and xyz
    assert (rest == want).all(), f"{int((rest != want).sum())} words outside mean_dist2 and temp were written"
    return [got[arena.slices[o]] for o in outs]


def _assert_matches(name, rows=None):
    p, (want, _) = scene(name), reference_of(name)
    if rows is not None:
        p, want = p[rows], want[rows]                               # (the result belongs to the point, wherever its row is)
    first, second = _run(p)
    bad = np.nonzero(first != _bits(want))[0]
    assert bad.size == 0, (f"{name}: {bad.size} of {p.shape[0]} differ, first rows {bad[:6].tolist()}: got "
                           f"{first[bad[:6]].view(F).tolist()}, want {want[bad[:6]].tolist()}")
    assert (first == second).all(), f"{name}: two runs differ"
    return first.view(F)


@pytest.mark.parametrize("n", SIZES)
def test_mean_dist2_is_the_brute_force_bit_for_bit_at_every_size(n):
    """1 .. 5: the means over fewer than three neighbours; around a leaf (one wave) and around a node's worth of leaves; 3 nodes and a bit."""
    _assert_matches(f"uniform_{n}")


@pytest.mark.parametrize("name", sorted(SCENES))
def test_mean_dist2_is_the_brute_force_bit_for_bit_on_every_scene(name):
    got = _assert_matches(name)
    if name == "identical":
        assert (_bits(got) == 0).all()                               # +0 everywhere
    if name == "lattice":
        assert (got == 1.0).all()


def test_shuffled_rows_give_every_point_the_same_result():
    rows = np.random.default_rng(12).permutation(scene("uniform_4097").shape[0])
    _assert_matches("uniform_4097", rows)
    _assert_matches("uniform_4097", rows[::-1].copy())


def _same_bits(t, a):
    return tuple(t.shape) == a.shape and (_bits(t.detach().cpu().numpy()) == _bits(a)).all()


def test_python_wrappers_against_the_same_expressions_on_the_reference():
    """knn_mean_dist2 and initial_values: the reference's mean_dist2 uploaded and carried through the SAME torch operations on
    the same device, so that no logarithm is compared across implementations."""
    import math
    import torch
    from gsrast_amd import init
    p, (want, _) = scene("coincident"), reference_of("coincident")
    n = p.shape[0]
    xyz = torch.from_numpy(p.copy()).cuda()
    rgb = torch.from_numpy(np.random.default_rng(13).uniform(0.0, 1.0, (n, 3)).astype(F)).cuda()
    assert _same_bits(init.knn_mean_dist2(xyz), want)
    wide = torch.zeros((n, 5), dtype=torch.float32, device="cuda")
    wide[:, 1:4] = xyz
    assert _same_bits(init.knn_mean_dist2(wide[:, 1:4]), want)        # (a strided view is copied)
    assert tuple(init.knn_mean_dist2(xyz[:0]).shape) == (0,)
    got_xyz, opacity_logit, log_scale, rotation, shs = init.initial_values(xyz, rgb)
    assert got_xyz is xyz and _same_bits(xyz, p)
    ref = torch.from_numpy(want.copy()).cuda()
    assert (want < 1e-7).any() and (want > 1e-7).any()               # (both sides of the clamp)
    column = torch.log(torch.sqrt(torch.clamp_min(ref, 1e-7)))
    assert _same_bits(log_scale, column[:, None].repeat(1, 3).cpu().numpy())
    assert _same_bits(rotation, np.tile(F([1, 0, 0, 0]), (n, 1)))
    assert _same_bits(opacity_logit, np.full(n, math.log(0.1 / 0.9), F))
    want_shs = torch.zeros((n, 48), dtype=torch.float32, device="cuda")
    want_shs[:, 0:3] = (rgb - 0.5) / 0.28209479177387814
    assert _same_bits(shs, want_shs.cpu().numpy())


def test_from_points_through_one_training_step(tmp_path):
    import torch
    from helpers import posed_camera
    from gsrast_amd.autograd import FrameSlot, GaussianParams, render
    from gsrast_amd.loss import photometric_loss
    from gsrast_amd.optim import GaussianAdam
    from gsrast_amd.rasterizer import SplatRasterizer
    RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
    rng = np.random.default_rng(14)
    xyz = rng.uniform(-1.0, 1.0, (500, 3)).astype(F)
    rgb = rng.integers(0, 256, (500, 3)).astype(np.uint8)
    params = GaussianParams.from_points(xyz, rgb)
    assert params.num_gaussians == 500 and _same_bits(params.xyz, xyz)
    want = torch.log(torch.sqrt(torch.clamp_min(torch.from_numpy(reference_of_points(xyz)).cuda(), 1e-7)))
    assert _same_bits(params.log_scale[:, 2], want.cpu().numpy())
    dc = (torch.from_numpy(rgb).cuda().to(torch.float32) / 255.0 - 0.5) / 0.28209479177387814
    assert _same_bits(params.shs[:, :3], dc.cpu().numpy())
    with pytest.raises(ValueError, match="not finite"):
        GaussianParams.from_points(np.where(np.arange(1500).reshape(500, 3) == 7, np.nan, xyz).astype(F), rgb)

    path = str(tmp_path / "initial.ply")
    params.save_ply(path)
    again = GaussianParams.from_ply(path)
    for k in RAW:
        assert _same_bits(getattr(again, k), getattr(params, k).detach().cpu().numpy()), k

    rast, slot = SplatRasterizer(64, 64), FrameSlot()
    opt = GaussianAdam([getattr(params, k) for k in RAW], lr=1e-3)
    before = [getattr(params, k).detach().clone() for k in RAW]
    color, _, _ = render(params, rast, posed_camera(64, 64, eye=(2.0, -1.2, -4.2), target=(0.0, 0.0, 0.0), roll=0.4), radii_slot=slot)
    target = torch.from_numpy(rng.uniform(0.0, 1.0, (3, 64, 64)).astype(F)).cuda()
    loss = photometric_loss(color, target)
    loss.backward()
    assert bool(torch.isfinite(loss)) and bool((slot.radii > 0).any())
    for k in RAW:
        g = getattr(params, k).grad
        assert g is not None and bool(torch.isfinite(g).all()), k
    assert bool((params.xyz.grad != 0).any())
    opt.step(slot.radii)
    assert any(not torch.equal(b, getattr(params, k).detach()) for b, k in zip(before, RAW))
    assert all(bool(torch.isfinite(getattr(params, k)).all()) for k in RAW)


def reference_of_points(xyz):
    import knn_ref
    return knn_ref.mean_dist2(xyz)


def test_from_points_ply_reads_the_upstream_layout(tmp_path):
    from gsrast_amd.autograd import GaussianParams
    from test_knn_cpu import _write_points
    rng = np.random.default_rng(15)
    xyz, rgb = rng.normal(size=(130, 3)).astype(F), rng.integers(0, 256, (130, 3)).astype(np.uint8)
    path = str(tmp_path / "points3D.ply")
    _write_points(path, xyz, rgb, normals=True)
    a, b = GaussianParams.from_points_ply(path), GaussianParams.from_points(xyz, rgb)
    for k in ("xyz", "opacity_logit", "log_scale", "rotation", "shs"):
        assert _same_bits(getattr(a, k), getattr(b, k).detach().cpu().numpy()), k


def test_a_launching_call_after_a_refusal_leaves_no_error():
    """The pattern of tests/test_gpu_error_contract.py for the one entry point of include/gsrast_amd_init.h whose success is a
    launch: after another entry point was refused, a valid call returns GSR_OK, leaves GSR_OK and no HIP text."""
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    n = 2 * _capi.GSR_KNN_LEAF * _capi.GSR_KNN_NODE + 5                    # (every kernel of the call has more than one workgroup's work or node)
    xyz = torch.from_numpy(scene(f"uniform_{n}").copy()).cuda()
    out = torch.zeros(n, dtype=torch.float32, device="cuda")
    temp = torch.zeros(int(L.gsr_knn_temp_bytes(n)), dtype=torch.uint8, device="cuda")
    a = _capi.ForwardArgs(struct_size=C.sizeof(_capi.ForwardArgs))
    assert L.gsr_forward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_knn_mean_dist2(n, xyz.data_ptr(), out.data_ptr(), temp.data_ptr(), _capi.stream(xyz.device)) == _capi.GSR_OK
    assert L.gsr_last_error() == _capi.GSR_OK and L.gsr_last_hip_error() == b""
    torch.cuda.synchronize()
    assert bool((out > 0).all())
