"""GPU: the 3D smoothing filter (include/gsrast_amd_filter3d.h, gsrast_amd/filter3d.py, render(..., filter_3d=values)).
observe, finalize and forward bit for bit against the float32 restatements of tests/filter3d_ref.py, the backward against its
float64 autograd function within one float32 ulp, and the composition with the library: image bits, raw-parameter gradients,
the default path untouched, Filter3D against the reference, remap across a densification, a short training run, the fused .ply.
The references' own preconditions are tests/test_filter3d_cpu.py's."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import antialias_ref as AR
import filter3d_ref as R

pytestmark = pytest.mark.gpu

F = np.float32
PAD = 64                        # floats of sentinel on each side of every array written (256 bytes: the rows stay 16-byte aligned)
SENTINEL = -777.25
SIZES = [1, 63, 64, 65, 255, 256, 257]


def _torch():
    import torch
    return torch


def _capi():
    from gsrast_amd import _capi
    return _capi


def _dev(a, dtype=np.float32):
    return _torch().from_numpy(np.array(a, dtype)).cuda()           # (a copy: shared, read-only references stay as they are)


def _bits(t):
    torch = _torch()
    t = t.detach() if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t))
    return t.contiguous().view(torch.int32).cpu().numpy()


def _same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and bool((_bits(a) == _bits(b)).all())


class _Guarded:
    """A device array of `floats` floats between two runs of sentinels; `init`: its initial contents."""

    def __init__(self, floats, init=None):
        self.buf = _torch().full((floats + 2 * PAD,), SENTINEL, dtype=_torch().float32, device="cuda")
        self.floats = floats
        if init is not None:
            self.buf[PAD:PAD + floats] = _dev(init).reshape(-1)

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * PAD

    def inner(self):
        return self.buf[PAD:PAD + self.floats]

    def intact(self):
        return bool((self.buf[:PAD] == SENTINEL).all()) and bool((self.buf[PAD + self.floats:] == SENTINEL).all())


def _ready():
    """The guarded arrays are filled on torch's current stream and a call may run on another one: everything enqueued so far is
    finished before the call is made."""
    _torch().cuda.synchronize()


def _stream(stream):
    return stream if stream is not None else _torch().cuda.current_stream().cuda_stream


# ---- the plain C calls into guarded arrays ---------------------------------------------------------------------------------------------
def _observe(pos_dev, rec_dev, min_depth=None, stream=None):
    """min_depth [N] (a device tensor) after one gsr_filter3d_observe over rec_dev, starting from `min_depth` (numpy) or +inf."""
    capi = _capi()
    n, stride = int(pos_dev.shape[0]), int(pos_dev.shape[1])
    md = _Guarded(n, np.full(n, np.inf, F) if min_depth is None else min_depth)
    a = capi.Filter3dObserveArgs()
    a.struct_size, a.flags, a.num_gaussians, a.position_stride, a.num_cameras = C.sizeof(a), 0, n, stride, int(rec_dev.shape[0])
    a.positions, a.cameras, a.min_depth, a.stream = pos_dev.data_ptr(), rec_dev.data_ptr(), md.ptr, _stream(stream)
    _ready()
    capi.call("gsr_filter3d_observe", C.byref(a))
    _torch().cuda.synchronize()
    assert md.intact(), "a write outside min_depth"
    return md.inner()


def _finalize(min_depth, max_focal):
    capi, torch = _capi(), _torch()
    n = len(min_depth)
    md, out = _dev(min_depth), _Guarded(n)
    nbytes = int(capi.lib().gsr_filter3d_temp_bytes(n))
    assert nbytes % 4 == 0
    temp = torch.full((nbytes + 512,), 0xFF, dtype=torch.uint8, device="cuda")          # exactly as long as asked for, between guard bytes
    a = capi.Filter3dFinalizeArgs()
    a.struct_size, a.flags, a.num_gaussians, a.max_focal = C.sizeof(a), 0, n, max_focal
    a.min_depth, a.filter, a.temp, a.temp_bytes, a.stream = md.data_ptr(), out.ptr, temp.data_ptr() + 256, nbytes, _stream(None)
    before = md.clone()
    _ready()
    capi.call("gsr_filter3d_finalize", C.byref(a))
    torch.cuda.synchronize()
    assert out.intact(), "a write outside filter"
    assert bool((temp[:256] == 0xFF).all()) and bool((temp[256 + nbytes:] == 0xFF).all()), "a write outside temp"
    assert _same_bits(before, md), "min_depth was written"
    return out.inner()


def _forward(scales, opacities, filt, outputs=("s", "o"), stream=None):
    capi = _capi()
    n = int(opacities.shape[0])
    out = {"s": _Guarded(4 * n), "o": _Guarded(n)}
    a = capi.Filter3dArgs()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), 0, n
    a.scales, a.opacities, a.filter = scales.data_ptr(), opacities.data_ptr(), filt.data_ptr()
    a.scales_out = out["s"].ptr if "s" in outputs else None
    a.opacities_out = out["o"].ptr if "o" in outputs else None
    a.stream = _stream(stream)
    _ready()
    capi.call("gsr_filter3d_forward", C.byref(a))
    _torch().cuda.synchronize()
    assert all(g.intact() for g in out.values()), "a write outside an output array"
    for k, g in out.items():
        if k not in outputs:
            assert bool((g.inner() == SENTINEL).all()), "an output that was not asked for was written"
    return {"s": out["s"].inner().reshape(n, 4), "o": out["o"].inner()}


def _backward(scales, opacities, filt, g_s, g_o, radii, outputs=("s", "o")):
    capi = _capi()
    n = int(opacities.shape[0])
    out = {"s": _Guarded(4 * n), "o": _Guarded(n)}
    a = capi.Filter3dBackwardArgs()
    a.struct_size, a.flags, a.num_gaussians = C.sizeof(a), 0, n
    a.scales, a.opacities, a.filter = scales.data_ptr(), opacities.data_ptr(), filt.data_ptr()
    p = lambda t: t.data_ptr() if t is not None else None
    a.dL_dscales_out, a.dL_dopacities_out, a.radii = p(g_s), p(g_o), p(radii)
    a.dL_dscales = out["s"].ptr if "s" in outputs else None
    a.dL_dopacities = out["o"].ptr if "o" in outputs else None
    a.stream = _stream(None)
    _ready()
    capi.call("gsr_filter3d_backward", C.byref(a))
    _torch().cuda.synchronize()
    assert all(g.intact() for g in out.values()), "a write outside an output array"
    for k, g in out.items():
        if k not in outputs:
            assert bool((g.inner() == SENTINEL).all()), "an output that was not asked for was written"
    return {"s": out["s"].inner().reshape(n, 4), "o": out["o"].inner()}


# ---- observe ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _many_records():
    """chunk + 1 camera records (shared, left unchanged): a chunk of cameras around a cloud, and one inside it, so that the
    second chunk's only camera is the nearest to some points."""
    from gsrast_amd import filter3d
    from gsrast_amd.camera import first_person_camera
    chunk = _capi().GSR_FILTER3D_CAMERA_CHUNK
    inside = first_person_camera((0.3, 0.2, -1.0), 0.1, 0.05, math.radians(45.0), 0.05, 50.0, 96, 64)
    rec, max_focal = filter3d.camera_records(R.orbit_cameras(chunk, seed=4) + [inside])
    rec.setflags(write=False)
    return rec, max_focal


@pytest.mark.parametrize("n", SIZES)
def test_observe_is_the_restatement_at_every_size(n):
    """N around the wave and the workgroup; 1, 2, chunk - 1, chunk and chunk + 1 cameras (one chunk, its last lane, two chunks);
    both strides. The fourth float of a means3D row is not read: it holds a NaN."""
    chunk = _capi().GSR_FILTER3D_CAMERA_CHUNK
    rec, _ = _many_records()
    for stride in (3, 4):
        pts = R.seeded_points(n, seed=n, spread=5.0, stride=stride)
        if stride == 4:
            pts[:, 3] = np.nan
        pos = _dev(pts)
        for cams in (1, 2, chunk - 1, chunk, chunk + 1):
            rec_dev = _dev(rec[:cams])
            want = R.observe_f32(pts, rec[:cams])
            got = _observe(pos, rec_dev)
            assert _same_bits(got, want), (n, stride, cams, int((_bits(got) != _bits(want)).sum()))
            assert _same_bits(pos, pts) and _same_bits(rec_dev, rec[:cams]), "an input was written"
    if n == 257:
        seen = want < np.inf
        assert seen.sum() >= 50 and (~seen).sum() >= 1
        # the last camera alone decides some rows: the second chunk is not idle
        assert (want != R.observe_f32(pts, rec[:chunk])).sum() >= 3


def _boundary_points():
    """Points for R.exact_camera() (t = (x, y, z), focal 512, 640 x 480: bounds -96, 736, -72, 552), and what each is meant to
    be. At t_2 = 1, px = 512 x + 320 and py = 512 y + 240 are exact. (A size that is a power of two has no bound -0.15 W that
    px can hit exactly: the bound has 24 significant bits below those of px - W/2. 640 x 480 makes all four bounds integers.)
    "Beyond" is the nearest position whose px (py) is the next float outside the bound: on the low sides the next position (its
    px, -96 - 2^-15, is exact); on the high sides the second next — the next one's px, 736 + 2^-15, is not a float32 and rounds
    back onto the bound, which is a case of its own."""
    up, dn = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    x_lo, x_hi, y_lo, y_hi = F(-416.0 / 512.0), F(416.0 / 512.0), F(-312.0 / 512.0), F(312.0 / 512.0)
    rows = [
        ("on x_lo", (x_lo, 0, 1), True), ("beyond x_lo", (dn(x_lo), 0, 1), False),
        ("on x_hi", (x_hi, 0, 1), True), ("rounds onto x_hi", (up(x_hi), 0, 1), True), ("beyond x_hi", (up(up(x_hi)), 0, 1), False),
        ("on y_lo", (0, y_lo, 1), True), ("beyond y_lo", (0, dn(y_lo), 1), False),
        ("on y_hi", (0, y_hi, 1), True), ("rounds onto y_hi", (0, up(y_hi), 1), True), ("beyond y_hi", (0, up(up(y_hi)), 1), False),
        ("a corner", (x_lo, y_hi, 1), True),
        ("at 0.2", (0, 0, F(0.2)), False), ("above 0.2", (0, 0, up(0.2)), True),
        ("between 0.001 and 0.2", (0.001, 0.001, 0.05), False), ("below 0.001", (0, 0, 0.0005), False),
        ("behind", (0, 0, -2), False), ("behind, off axis", (0.5, 0.5, -2), False),
        ("NaN x", (np.nan, 0, 1), False), ("NaN y", (0, np.nan, 1), False), ("NaN z", (0, 0, np.nan), False),
        ("+inf x", (np.inf, 0, 1), False), ("-inf y", (0, -np.inf, 1), False), ("+inf z", (0, 0, np.inf), False),
        ("-inf z", (0, 0, -np.inf), False), ("inf x and z", (np.inf, 0, np.inf), False),
        ("centre", (0, 0, 4), True),
    ]
    return [r[0] for r in rows], np.array([r[1] for r in rows], F), np.array([r[2] for r in rows])


def test_observe_decides_every_boundary_as_the_header_says():
    from gsrast_amd import filter3d
    names, pts, meant = _boundary_points()
    rec, _ = filter3d.camera_records([R.exact_camera()])
    want, detail = R.observe_f32(pts, rec, detail=True)
    d = detail[0]
    at = names.index
    # each case occurs, by the reference's own masks
    assert np.array_equal(d["valid"], meant), [n for n, v, m in zip(names, d["valid"], meant) if v != m]
    for side, key, bound in (("x_lo", "px", -96.0), ("x_hi", "px", 736.0), ("y_lo", "py", -72.0), ("y_hi", "py", 552.0)):
        assert d[key][at("on " + side)] == bound
        beyond = d[key][at("beyond " + side)]
        assert beyond == (F(bound) - F(2.0 ** -15) if side.endswith("lo") else np.nextafter(F(bound), F(np.inf)))
        assert not d["in_" + side][at("beyond " + side)] and d["depth_ok"][at("beyond " + side)]
    assert d["t2"][at("at 0.2")] == F(0.2) and not d["depth_ok"][at("at 0.2")] and d["depth_ok"][at("above 0.2")]
    inside = d["in_x_lo"] & d["in_x_hi"] & d["in_y_lo"] & d["in_y_hi"]
    assert inside[at("between 0.001 and 0.2")] and inside[at("below 0.001")] and inside[at("behind")]
    assert not inside[at("behind, off axis")]              # (divided by 0.001: far off the screen)
    assert np.isnan(d["px"][at("NaN x")]) and np.isnan(d["t2"][at("NaN z")]) and np.isnan(d["px"][at("inf x and z")])
    assert d["px"][at("rounds onto x_hi")] == 736.0 and d["py"][at("rounds onto y_hi")] == 552.0
    # (+inf z: the zero entries of the rotation's other rows times inf are NaN: t_0 and t_1 are NaN, the pair is invalid)
    assert d["depth_ok"][at("+inf z")] and np.isnan(d["px"][at("+inf z")])
    assert want[at("+inf z")] == np.inf and want[at("above 0.2")] == np.nextafter(F(0.2), F(1))
    for stride in (3, 4):
        p = np.ones((len(pts), stride), F)
        p[:, :3] = pts
        got = _observe(_dev(p), _dev(rec))
        assert _same_bits(got, want), [names[i] for i in np.nonzero(_bits(got) != _bits(want))[0]]


def test_observe_accumulates_exactly_in_any_batching_and_order():
    torch = _torch()
    chunk = _capi().GSR_FILTER3D_CAMERA_CHUNK
    rec, _ = _many_records()
    n = 300
    pts = R.seeded_points(n, seed=8, spread=5.0)
    pos = _dev(pts)
    whole = _observe(pos, _dev(rec))
    assert _same_bits(whole, R.observe_f32(pts, rec))
    a, b = rec[:chunk // 2], rec[chunk // 2:]
    a_then_b = _observe(pos, _dev(b), min_depth=_observe(pos, _dev(a)).cpu().numpy())
    b_then_a = _observe(pos, _dev(a), min_depth=_observe(pos, _dev(b)).cpu().numpy())
    shuffled = _observe(pos, _dev(rec[np.random.default_rng(2).permutation(len(rec))]))
    assert _same_bits(a_then_b, whole) and _same_bits(b_then_a, whole) and _same_bits(shuffled, whole)
    assert _same_bits(_observe(pos, _dev(rec), min_depth=whole.cpu().numpy()), whole)          # a repeated call changes nothing
    # a running minimum that is not +inf is respected: below every depth it stays, above it gives way
    start = np.where(np.arange(n) % 2 == 0, F(0.25), F(1e6)).astype(F)
    got = _observe(pos, _dev(rec), min_depth=start)
    want = R.observe_f32(pts, rec, min_depth=start)
    assert _same_bits(got, want) and (want == F(0.25)).sum() >= n // 2 - 5 and ((want != F(1e6)) & (want != F(0.25))).sum() >= 50
    # on a second stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    assert _same_bits(_observe(pos, _dev(rec), stream=side.cuda_stream), whole)
    assert _same_bits(pos, pts), "an input was written"


# ---- finalize -----------------------------------------------------------------------------------------------------------------------
def test_finalize_fills_the_unseen_with_the_largest_seen_depth():
    inf = F(np.inf)
    rng = np.random.default_rng(12)
    cases = {
        "none seen": np.full(300, inf, F),
        "one seen": np.where(np.arange(300) == 137, F(3.5), inf).astype(F),
        "all seen": rng.uniform(0.21, 40.0, 300).astype(F),
        "N = 1, seen": np.array([2.0], F),
        "N = 1, unseen": np.array([inf], F),
    }
    # the only maximum sits in the last, partial wave (rows 256 ..: a second workgroup of one wave with 44 live lanes)
    last = np.where(rng.uniform(size=300) < 0.5, rng.uniform(0.21, 5.0, 300), np.inf).astype(F)
    last[297] = F(77.0)
    last[298:] = inf
    cases["maximum in the last partial wave"] = last
    for n in SIZES:
        cases[f"N = {n}"] = np.where(rng.uniform(size=n) < 0.3, np.inf, rng.uniform(0.21, 9.0, n)).astype(F)
    for name, md in cases.items():
        for focal in (512.0, 1234.5):
            want = R.finalize_f32(md, focal)
            got = _finalize(md, focal)
            assert _same_bits(got, want), (name, focal)
    assert (R.finalize_f32(cases["none seen"], 512.0).view(np.uint32) == 0).all()
    assert R.finalize_f32(last, 512.0)[299] == F(F(77.0) / F(512.0)) * R.K


# ---- forward ------------------------------------------------------------------------------------------------------------------------
FILTERS = np.array([0.0, 1e-30, 1e-3, 1.0, np.inf, np.nan], F)          # (1e-30 squared underflows to 0: IDENTITY)
EDGE_SCALES = np.array([0.0, 1e-20, 1.0, 1e9], F)


def _forward_case(n, seed=0):
    """Every combination of FILTERS with EDGE_SCALES in each axis first, then seeded rows; the fourth float is the activation
    kernel's e and other values; opacities include 0, 1 and a NaN."""
    rng = np.random.default_rng(seed)
    grid = np.array([[a, b, c, f] for f in FILTERS for a in EDGE_SCALES for b in EDGE_SCALES for c in EDGE_SCALES], F)
    scales = np.exp(rng.normal(-2.0, 1.5, (n, 4))).astype(F)
    filt = np.exp(rng.normal(-3.0, 1.5, n)).astype(F)
    filt[rng.uniform(size=n) < 0.15] = 0.0
    m = min(n, len(grid))
    pick = rng.permutation(len(grid))[:m] if n < len(grid) else np.arange(len(grid))
    scales[:m, :3], filt[:m] = grid[pick, :3], grid[pick, 3]
    scales[:, 3] = np.where(rng.uniform(size=n) < 0.5, F(np.e), rng.normal(size=n)).astype(F)
    scales[rng.uniform(size=n) < 0.1, 0] *= F(-1.0)
    o = rng.uniform(0.0, 1.0, n).astype(F)
    o[::7], o[3::11] = 0.0, 1.0
    if n > 5:
        o[5] = np.nan
    return scales, o, filt


@pytest.mark.parametrize("n", SIZES + [1000])
def test_forward_is_the_restatement_bit_for_bit(n):
    torch = _torch()
    scales, o, filt = _forward_case(n, seed=n)
    want = R.forward_f32(scales, o, filt)
    s_dev, o_dev, f_dev = _dev(scales), _dev(o), _dev(filt)
    got = _forward(s_dev, o_dev, f_dev)
    assert _same_bits(got["s"], want["scales_out"]), (n, np.nonzero((_bits(got["s"]) != _bits(want["scales_out"])).any(1))[0][:8])
    assert _same_bits(got["o"], want["opacities_out"]), (n, np.nonzero(_bits(got["o"]) != _bits(want["opacities_out"]))[0][:8])
    assert (_bits(got["s"])[:, 3] == scales[:, 3].view(np.int32)).all(), "the fourth float is carried"
    ident = want["identity"]
    assert (_bits(got["s"])[ident] == scales[ident].view(np.int32)).all() and (_bits(got["o"])[ident] == o[ident].view(np.int32)).all()
    only_s, only_o = _forward(s_dev, o_dev, f_dev, outputs=("s",)), _forward(s_dev, o_dev, f_dev, outputs=("o",))
    assert _same_bits(only_s["s"], got["s"]) and _same_bits(only_o["o"], got["o"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    other = _forward(s_dev, o_dev, f_dev, stream=side.cuda_stream)
    assert _same_bits(other["s"], got["s"]) and _same_bits(other["o"], got["o"])
    assert _same_bits(s_dev, scales) and _same_bits(o_dev, o) and _same_bits(f_dev, filt), "an input was written"
    if n == 1000:
        # every combination of the edge values is in the case, nothing of it is NaN but what a NaN opacity or scale makes so
        assert ident.sum() >= 3 * 64 and (~ident).sum() >= 3 * 64
        live = ~ident & ~np.isnan(o)
        assert np.isfinite(want["coef"][live]).all() and (want["coef"][live] == 0).any() and (want["coef"][live] > 0.99).any()
        assert not np.isnan(want["scales_out"][live, :3]).any() and np.isinf(want["scales_out"][live, :3]).any()


def test_python_smoothed_returns_the_calls_outputs():
    from gsrast_amd import filter3d
    scales, o, filt = _forward_case(300, seed=3)
    want = R.forward_f32(scales, o, filt)
    s, op = filter3d.smoothed(_dev(scales), _dev(o), _dev(filt))
    assert _same_bits(s, want["scales_out"]) and _same_bits(op, want["opacities_out"])
    with pytest.raises(ValueError):
        filter3d.smoothed(_dev(scales), _dev(o), _dev(filt[:-1]))
    with pytest.raises(ValueError):
        filter3d.smoothed(_dev(scales), _dev(o), _torch().from_numpy(filt))              # another device


# ---- backward -----------------------------------------------------------------------------------------------------------------------
def _backward_case(n, seed=21):
    """Seeded rows with finite, ordinary values (the float64 function is compared on them), among them rows with a zero scale in
    each axis, negative scales, IDENTITY filters (0 and one whose square underflows); a sixth of the radii <= 0, and five of
    those rows poisoned with NaN."""
    rng = np.random.default_rng(seed)
    scales = np.exp(rng.normal(-2.0, 1.5, (n, 4))).astype(F)
    scales[:, 3] = F(np.e)
    scales[rng.uniform(size=n) < 0.1, 1] *= F(-1.0)
    for j in range(3):
        scales[j::17, j] = 0.0
    filt = np.exp(rng.normal(-3.0, 1.5, n)).astype(F)
    filt[rng.uniform(size=n) < 0.1] = 0.0
    filt[rng.uniform(size=n) < 0.05] = F(1e-30)
    o = rng.uniform(0.01, 0.99, n).astype(F)
    g_s = rng.normal(size=(n, 4)).astype(F)
    g_o = rng.normal(size=n).astype(F)
    radii = rng.integers(1, 40, n).astype(np.int32)
    off = rng.uniform(size=n) < 1.0 / 6.0
    radii[off] = np.where(rng.uniform(size=off.sum()) < 0.5, 0, -1)
    poisoned = np.nonzero(off)[0][:5]
    scales[poisoned, :3] = np.nan
    g_s[poisoned[:3]] = np.nan
    g_o[poisoned[2:]] = np.nan
    return scales, o, filt, g_s, g_o, radii, poisoned


def _ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(F)
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)


def test_backward_is_the_float64_function_rounded_once():
    """The chain is evaluated in double and rounded once: within one float32 ulp of the float64 function's value rounded to
    float32 (the project's standing bound for such chains). dL/do = coef g_o is the float32 forward's coef: bit for bit."""
    n = 1000
    scales, o, filt, g_s, g_o, radii, poisoned = _backward_case(n)
    assert len(poisoned) == 5
    fwd = R.forward_f32(np.nan_to_num(scales), o, filt)
    ident, on = fwd["identity"], radii > 0
    assert (ident & on).sum() >= 50 and (~ident & on).sum() >= 500
    assert all(((scales[:, j] == 0) & on & ~ident).sum() >= 10 for j in range(3)) and ((scales[:, 1] < 0) & on & ~ident).sum() >= 30
    dev = [_dev(v) for v in (scales, o, filt, g_s, g_o)]
    before = [t.clone() for t in dev]
    rd = _dev(radii, np.int32)
    got = {k: v.cpu().numpy() for k, v in _backward(*dev, rd).items()}
    # culled rows: +0 everywhere, NaN inputs and all
    assert (got["s"][~on].view(np.uint32) == 0).all() and (got["o"][~on].view(np.uint32) == 0).all()
    assert (got["s"][:, 3].view(np.uint32) == 0).all()
    # IDENTITY rows pass g through bit for bit
    both = ident & on
    assert np.array_equal(got["s"][both, :3].view(np.uint32), g_s[both, :3].view(np.uint32))
    assert np.array_equal(got["o"][both].view(np.uint32), g_o[both].view(np.uint32))
    live = ~ident & on
    assert np.array_equal(got["o"][live].view(np.uint32), (fwd["coef"] * g_o)[live].view(np.uint32))
    ref = R.gradients64(scales[live], o[live], filt[live], g_s[live], g_o[live], identity=np.zeros(live.sum(), bool))
    want = ref["scales"].astype(F)
    err = np.abs(got["s"][live, :3].astype(np.float64) - want.astype(np.float64))
    worst = float((err / _ulp32(want)).max())
    print(f"[filter3d] dL_dscales: worst error {worst:.2f} ulp of the float64 value rounded to float32")
    assert np.isfinite(got["s"][on]).all() and (err <= _ulp32(want)).all(), worst
    assert np.allclose(got["o"][live], ref["opacities"], rtol=3e-7, atol=0)
    # a zero scale: its own gradient is g_s . 0 + 0 (sign(0) = 0), and the others lose the opacity's share (u = 0)
    zero0 = (scales[:, 0] == 0) & live
    assert (got["s"][zero0, 0] == 0).all()
    assert all(_same_bits(b, t) for b, t in zip(before, dev)), "an input was written"


def test_backward_outputs_alone_twice_without_radii_and_with_one_incoming_gradient():
    n = 257
    scales, o, filt, g_s, g_o, radii, _ = _backward_case(n, seed=22)
    dev = [_dev(v) for v in (scales, o, filt, g_s, g_o)]
    rd = _dev(radii, np.int32)
    both = _backward(*dev, rd)
    again = _backward(*dev, rd)
    assert all(_same_bits(both[k], again[k]) for k in both)
    for k in ("s", "o"):
        alone = _backward(*dev, rd, outputs=(k,))
        assert _same_bits(alone[k], both[k]), k
    # radii == NULL: every row is computed; the rows that had a tile are the same bits
    free = _backward(*dev, None)
    had = radii > 0
    for k in both:
        assert (_bits(free[k])[had] == _bits(both[k])[had]).all(), k
    finite_off = ~had & np.isfinite(g_o) & np.isfinite(scales[:, 0])
    assert finite_off.any() and (free["o"].cpu().numpy()[finite_off] != 0).any()
    # one incoming gradient: the other counts as zeros
    s_d, o_d, f_d, gs_d, go_d = dev
    zeros4, zeros1 = _torch().zeros_like(gs_d), _torch().zeros_like(go_d)
    only_gs, want_gs = _backward(s_d, o_d, f_d, gs_d, None, rd), _backward(s_d, o_d, f_d, gs_d, zeros1, rd)
    only_go, want_go = _backward(s_d, o_d, f_d, None, go_d, rd), _backward(s_d, o_d, f_d, zeros4, go_d, rd)
    ok = had & np.isfinite(g_o) & np.isfinite(g_s).all(1)
    for got, want in ((only_gs, want_gs), (only_go, want_go)):
        for k in got:
            a, b = got[k].cpu().numpy()[ok], want[k].cpu().numpy()[ok]
            assert np.array_equal(a, b), k               # (values: a zero product may be -0 where the NULL side writes +0)


# ---- through the library --------------------------------------------------------------------------------------------------------------
DRAW = dict(plan="sort", tile_history=False)
RAW = ("xyz", "opacity_logit", "log_scale", "rotation", "shs")
BG = (0.1, 0.2, 0.3)


def _params(semantics="inria"):
    from gsrast_amd.autograd import GaussianParams
    raw = AR.composition_raw(semantics)
    return GaussianParams.from_raw(*(raw[k] for k in RAW), sh_layout="coefficient_major" if semantics == "inria" else "file", device="cuda:0")


def _rasterizer():
    from gsrast_amd.rasterizer import SplatRasterizer
    return SplatRasterizer(AR.CW, AR.CH, background=BG)


@functools.lru_cache(maxsize=None)
def _weights():
    rng = np.random.default_rng(17)
    return _dev(rng.normal(size=(3, AR.CH, AR.CW))), _dev(1.0 + 0.25 * rng.normal(size=(AR.CH, AR.CW)))


def _loss(color, dmap):
    w, wd = _weights()
    return (w * color).sum() + (wd * dmap).sum()


def _training_cameras():
    """Five first_person_camera poses on one side of the composition scene, at its frame size (what lies behind them is seen by none)."""
    return R.orbit_cameras(5, width=AR.CW, height=AR.CH, radius=5.0, seed=6, arc=1.0)


@functools.lru_cache(maxsize=None)
def _filter_values():
    """The composition scene's filter over the training cameras, by the restatement, scaled up so that it matters at this
    frame's focal length (numpy float32 [N], a tenth of them zero: IDENTITY rows inside a frame)."""
    from gsrast_amd import filter3d
    raw = AR.composition_raw("inria")
    rec, max_focal = filter3d.camera_records(_training_cameras())
    v = R.finalize_f32(R.observe_f32(raw["xyz"], rec), max_focal) * F(4.0)
    v[::10] = 0.0
    v.setflags(write=False)
    return v


@pytest.mark.parametrize("antialiased", [False, True])
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_filtered_frame_is_the_frame_of_the_smoothed_values(semantics, antialiased):
    """render(filter_3d=v) against rasterize handed smoothed(...) values as leaves: the image bits, and the raw-parameter
    gradients against those leaves' gradients taken through the float64 smoothing and the activation reference."""
    import activation_ref as A
    torch = _torch()
    from gsrast_amd import autograd, filter3d
    cam, kw = AR.composition_camera(), dict(semantics=semantics, sh_degree=3, depth=True, antialiased=antialiased, **DRAW)
    v = _dev(_filter_values())
    params, rast, slot = _params(semantics), _rasterizer(), autograd.RadiiSlot()
    color, dmap, omap = autograd.render(params, rast, cam, filter_3d=v, radii_slot=slot, **kw)
    _loss(color, dmap).backward()
    with torch.no_grad():
        act = autograd.activate(params.xyz, params.opacity_logit, params.log_scale, params.rotation)
        s_sm, o_sm = filter3d.smoothed(act[1], act[3], v)
    scales, opac = act[1].cpu().numpy(), act[3].cpu().numpy()
    fwd = R.forward_f32(scales, opac, _filter_values())
    assert _same_bits(s_sm, fwd["scales_out"]) and _same_bits(o_sm, fwd["opacities_out"])
    leaves = [act[0].clone().requires_grad_(True), s_sm.clone().requires_grad_(True), act[2].clone().requires_grad_(True),
              o_sm.clone().requires_grad_(True)]
    shs = params.shs.detach().clone().requires_grad_(True)
    view, proj, cam_pos, tx, ty = autograd._camera_tensors(cam, rast.device)
    rast2, slot2 = _rasterizer(), autograd.RadiiSlot()
    color2, dmap2, omap2 = autograd.rasterize(rast2, *leaves, shs, view, proj, cam_pos, (tx, ty), radii_slot=slot2, **kw)
    assert _same_bits(color, color2) and _same_bits(dmap, dmap2) and _same_bits(omap, omap2)
    radii = slot.radii.cpu().numpy()
    assert np.array_equal(radii, slot2.radii.cpu().numpy()) and (radii > 0).sum() > 100 and (radii <= 0).sum() >= 10
    vis = radii > 0
    _loss(color2, dmap2).backward()
    # the frame is another one than the unfiltered frame
    plain = autograd.render(_params(semantics), _rasterizer(), cam, **kw)[0]
    assert not _same_bits(plain, color)
    # expected raw gradients: the leaves' through the float64 smoothing (culled rows: zero) and the activation reference
    g_s, g_o = leaves[1].grad.cpu().numpy(), leaves[3].grad.cpu().numpy()
    ref = R.gradients64(scales, opac, _filter_values(), np.where(vis[:, None], g_s, 0), np.where(vis, g_o, 0), identity=fwd["identity"])
    pad = lambda a: np.concatenate([a, np.zeros((a.shape[0], 4 - a.shape[1]))], 1)
    raw = AR.composition_raw(semantics)
    want = dict(zip(("xyz", "opacity_logit", "log_scale", "rotation"),
                    A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], leaves[0].grad.cpu().numpy().astype(np.float64),
                               pad(ref["scales"]), leaves[2].grad.cpu().numpy().astype(np.float64), ref["opacities"], radii=radii)))
    without = dict(zip(("xyz", "opacity_logit", "log_scale", "rotation"),
                       A.backward(raw["opacity_logit"], raw["log_scale"], raw["rotation"], leaves[0].grad.cpu().numpy().astype(np.float64),
                                  g_s.astype(np.float64), leaves[2].grad.cpu().numpy().astype(np.float64), g_o.astype(np.float64), radii=radii)))
    for k, w in want.items():
        got = getattr(params, k).grad.cpu().numpy().astype(np.float64)
        top = float(np.abs(w).max())
        err = float(np.abs(got - w).max()) / top
        share = float(np.abs(without[k] - w).max()) / top
        print(f"[filter3d] {semantics} antialiased={antialiased} {k}.grad: error {err:.2e} of the largest entry {top:.3e}; "
              f"without the smoothing's gradient {share:.2e}")
        # two float32 roundings (the smoothing's output, the activation's) of a chain evaluated in double: 4 x 2^-24 of the largest entry
        assert top > 0 and err <= 4.0 * 2.0 ** -24, (k, err)
        if k in ("opacity_logit", "log_scale"):
            assert share > 1e-3, (k, share)              # a backward that dropped the smoothing would show
        assert (got[~vis] == 0).all(), k
    assert _same_bits(params.shs.grad, shs.grad)


@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_default_path_is_untouched_and_a_zero_filter_is_no_filter(semantics):
    torch = _torch()
    from gsrast_amd import autograd
    cam, kw = AR.composition_camera(), dict(semantics=semantics, sh_degree=3, depth=True, **DRAW)
    n = AR.CN
    runs = []
    for extra in ({}, {"filter_3d": None}, {"filter_3d": torch.zeros(n, device="cuda")}):
        params = _params(semantics)
        color, dmap, omap = autograd.render(params, _rasterizer(), cam, **kw, **extra)
        _loss(color, dmap).backward()
        runs.append([color, dmap, omap] + [getattr(params, k).grad for k in RAW])
    assert all(_same_bits(a, b) for a, b in zip(runs[0], runs[1]))
    assert all(_same_bits(a, b) for a, b in zip(runs[0][:3], runs[2][:3]))
    # (the gradients under an all-zero filter are the default's values: they pass through the smoothing's backward unchanged)
    assert all(bool((a == b).all()) for a, b in zip(runs[0][3:], runs[2][3:]))
    for bad in (torch.zeros(n - 1, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.float64), torch.zeros(n)):
        with pytest.raises(ValueError):
            autograd.render(_params(semantics), _rasterizer(), cam, filter_3d=bad, **kw)


def test_filter3d_class_computes_the_reference_and_remaps_across_a_densification():
    torch = _torch()
    from gsrast_amd import autograd, filter3d
    from gsrast_amd.densify import DensityStats, densify_and_prune
    from gsrast_amd.optim import GaussianAdam
    params, cams = _params("inria"), _training_cameras()
    n = params.num_gaussians
    rec, max_focal = filter3d.camera_records(cams)
    md = R.observe_f32(AR.composition_raw("inria")["xyz"], rec)
    want = R.finalize_f32(md, max_focal)
    assert 10 <= (md == np.inf).sum() <= n // 2
    f = filter3d.Filter3D(n, "cuda:0")
    assert f.values is None
    got = f.compute(params, cams)
    assert got is f.values and _same_bits(got, want) and f.max_focal == max_focal
    # in batches, from means3D rows, and again: the same bits in a new tensor
    f2 = filter3d.Filter3D(n, "cuda:0")
    with torch.no_grad():
        means3D = params.activated()[0]
    f2.observe(means3D, cams[3:])
    f2.observe(params.xyz, cams[:3])
    again = f2.finalize()
    assert _same_bits(again, want) and again.data_ptr() != got.data_ptr() and _same_bits(f2.min_depth, md)
    with pytest.raises(ValueError):
        f.observe(params.xyz[:-1], cams)
    with pytest.raises(ValueError):
        filter3d.Filter3D(n, "cuda:0").finalize()
    # a densification: the filter follows its rows until the next compute
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": 1e-3} for k in RAW])
    stats = DensityStats(n, "cuda:0")
    slot = autograd.FrameSlot()
    cam = AR.composition_camera()
    color = autograd.render(params, _rasterizer(), cam, semantics="inria", sh_degree=3, radii_slot=slot, filter_3d=f.values)[0]
    color.sum().backward()
    stats.update(slot, AR.CW, AR.CH)
    src_of, (kept, clones, splits, total) = densify_and_prune(params, opt, stats, max_grad=1e-5, extent=4.0)
    assert total != n and clones + splits > 0 and params.num_gaussians == total
    old = f.values.clone()
    new = f.remap(src_of)
    assert new is f.values and tuple(new.shape) == (total,) and f.n == total
    assert np.array_equal(_bits(new), _bits(old)[src_of.cpu().numpy()])
    color = autograd.render(params, _rasterizer(), cam, semantics="inria", sh_degree=3, filter_3d=f.values)[0]
    assert bool(torch.isfinite(color).all())
    fresh = f.compute(params, cams)
    rec_xyz = params.xyz.detach().cpu().numpy()
    assert _same_bits(fresh, R.finalize_f32(R.observe_f32(rec_xyz, rec), max_focal))


def test_five_filtered_training_steps():
    torch = _torch()
    from gsrast_amd import autograd, filter3d
    from gsrast_amd.optim import GaussianAdam
    semantics = "inria"
    cam, rast, cams = AR.composition_camera(), _rasterizer(), _training_cameras()
    kw = dict(semantics=semantics, sh_degree=3, antialiased=True)
    with torch.no_grad():
        target = autograd.render(_params(semantics), rast, cam, **kw)[0]
    params = _params(semantics)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, amp in (("xyz", 0.02), ("opacity_logit", 0.5), ("log_scale", 0.2), ("rotation", 0.1), ("shs", 0.1)):
            p = getattr(params, k)
            p.add_((amp * torch.randn(p.shape, generator=gen)).to(p.device))
    rates = {"xyz": 1e-3, "opacity_logit": 2.5e-2, "log_scale": 1e-2, "rotation": 5e-3, "shs": 5e-3}
    opt = GaussianAdam([{"params": [getattr(params, k)], "lr": lr} for k, lr in rates.items()])
    f = filter3d.Filter3D(params.num_gaussians, "cuda:0")
    slot, losses = autograd.RadiiSlot(), []
    for step in range(5):
        if step in (0, 3):
            f.compute(params, cams)
        opt.zero_grad(set_to_none=True)
        loss = (autograd.render(params, rast, cam, radii_slot=slot, filter_3d=f.values, **kw)[0] - target).abs().mean()
        losses.append(float(loss.detach()))
        loss.backward()
        culled = slot.radii <= 0
        assert int(culled.sum()) >= 10
        for k in RAW:
            grad = getattr(params, k).grad
            assert bool(torch.isfinite(grad).all()) and bool((grad[culled] == 0).all()), k
        opt.step(slot.radii)
    print(f"[filter3d] L1 loss over five steps: {' '.join(f'{v:.6f}' for v in losses)}")
    assert all(np.isfinite(losses)) and losses[0] > 0


def test_fused_ply_shows_the_filtered_scene(tmp_path):
    """A save_fused_ply file, loaded by load_ply, against render(filter_3d=v), semantics fixed, antialiased=False. The file
    holds log(s') and logit(o'), and the loader's exp and sigmoid do not return s' and o' bit for bit, so the images are not
    compared by bits: the distance is held to what the same round trip costs WITHOUT a filter (an all-zero filter: the file
    then holds log and logit of the activated values, the round trip profiles/r06_ply_path.txt measures at full size: scales
    within 8 ulp, opacities within 5.96e-8, all but 12 of 2 073 600 pixels within 1e-4). Here: the scales within
    (|log s'| + 4) x 2^-24 relative with |log s'| <= 8 (the logarithm's rounding taken through the exponential, and both
    functions' own), the opacities within 2^-19 (the logit's rounding at |logit| <= 16 through a slope of at most 1/4, and both
    functions' own), every pixel within 1e-4, the library's parity criterion.
    Measured on one MI355X (printed by the test): filtered, scales within 3.05e-07 relative, opacities within 5.96e-08, image
    within 2.09e-07; without a filter 5.10e-07, 5.96e-08 and 2.98e-07; the filter itself moves the image by 2.28e-01."""
    torch = _torch()
    from gsrast_amd import autograd, filter3d, ply
    from gsrast_amd.rasterizer import SplatRasterizer
    semantics = "inria"
    cam, kw = AR.composition_camera(), dict(semantics=semantics, sh_degree=3, **DRAW)
    params = _params(semantics)
    report = {}
    for name, v in (("filtered", _dev(_filter_values())), ("no filter", torch.zeros(params.num_gaussians, device="cuda"))):
        with torch.no_grad():
            want = autograd.render(params, _rasterizer(), cam, filter_3d=v, **kw)[0]
            plain = autograd.render(params, _rasterizer(), cam, **kw)[0]
            act = params.activated()
            s_sm, o_sm = filter3d.smoothed(act[1], act[3], v)
        path = str(tmp_path / f"fused_{len(report)}.ply")
        filter3d.save_fused_ply(params, v, path)
        n, _ = ply.parse_header(path)
        assert n == params.num_gaussians
        scene = ply.load_ply(path, sh_layout="coefficient_major")
        assert _same_bits(scene["means3D"], act[0]) and _same_bits(scene["shs"], params.shs)
        assert float(s_sm[:, :3].log().abs().max()) <= 8.0 and float(torch.log(o_sm / (1 - o_sm)).abs().max()) <= 16.0
        rel_s = float(((scene["scales"][:, :3] - s_sm[:, :3]).abs() / s_sm[:, :3]).max())
        abs_o = float((scene["opacities"] - o_sm).abs().max())
        rast = SplatRasterizer(AR.CW, AR.CH, background=BG)
        rast.configure_from_scene(scene)
        got = rast.draw(cam, semantics=semantics, sh_degree=3, **DRAW)
        dist, moved = float((got - want).abs().max()), float((plain - want).abs().max())
        report[name] = (rel_s, abs_o, dist, moved)
        print(f"[filter3d] fused .ply, {name}: scales within {rel_s:.2e} relative, opacities within {abs_o:.2e}, image max "
              f"|difference| {dist:.3e} (the filter itself moves the image by {moved:.3e})")
    for name, (rel_s, abs_o, dist, moved) in report.items():
        assert rel_s <= 12.0 * 2.0 ** -24 and abs_o <= 2.0 ** -19 and dist <= 1e-4, (name, rel_s, abs_o, dist)
    assert report["no filter"][3] == 0.0 and report["filtered"][3] > 100 * max(report["filtered"][2], 1e-6)
