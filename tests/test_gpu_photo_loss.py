"""GPU: gsr_photo_loss_forward / _backward called directly — dL_dimage bit for bit against the float32 restatement
(tests/ssim_ref.py) over shapes from one pixel to several tiles, every lambda and upstream scalar, inside an arena of
sentinels; the three loss terms within a float32 ulp and reproducible — then gsrast_amd.loss.photometric_loss against those
direct calls (values, gradient, ownership, what it copies and refuses), and the loss at the end of a rendered frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import ssim_ref as R

pytestmark = pytest.mark.gpu

# (C, H, W): one pixel; smaller than the window; the window; one tile exactly, one channel; rows that are no multiple of
# 16 bytes with a partial tile both ways; several tiles and a partial one both ways, odd width (the float-by-float staging)
SHAPES = [(3, 1, 1), (3, 7, 5), (3, 11, 11), (1, 16, 64), (3, 33, 65), (3, 131, 197)]
LAMBDAS = (0.0, 0.2, 1.0)
UPS = (1.0, 0.37)
SENTINEL = -7.0
GAP = 64                                 # sentinel floats on both sides of every array


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _images(shape):
    x, y = R.images(shape, 1000 + sum(shape))
    for a in (x, y):
        a.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def _expected(shape, lam, up):
    """(gradient f32[C,H,W], (loss, l1, ssim) as doubles) of the restatement on _images(shape)."""
    x, y = _images(shape)
    grad = R.gradient(x, y, lam, up)
    grad.setflags(write=False)
    return grad, R.terms(x, y, lam)


class _Arena:
    """One device buffer filled with a sentinel; image, target, scratch, out, up and grad are 16-byte-aligned slices of it,
    GAP sentinel floats on both sides of each."""

    def __init__(self, x, y, up):
        import torch
        from gsrast_amd import _capi
        c, h, w = x.shape
        scratch_bytes = _capi.lib().gsr_photo_loss_scratch_bytes(c, w, h)
        assert scratch_bytes >= 12 * x.size + 16
        sizes = {"image": x.size, "target": x.size, "scratch": (scratch_bytes + 3) // 4, "out": 3, "up": 1, "grad": x.size}
        self.slices, at = {}, GAP
        for name, n in sizes.items():
            self.slices[name] = slice(at, at + n)
            at += (n + 3) // 4 * 4 + GAP
        host = np.full(at, SENTINEL, np.float32)
        host[self.slices["image"]], host[self.slices["target"]], host[self.slices["up"]] = x.reshape(-1), y.reshape(-1), up
        self.host = host
        self.dev = torch.from_numpy(host.copy()).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.shape = x.shape

    def ptr(self, name):
        p = self.dev.data_ptr() + 4 * self.slices[name].start
        assert p % 16 == 0
        return p

    def args(self, lam, want_backward=1):
        import torch
        from gsrast_amd import _capi
        a = _capi.PhotoLossArgs()
        a.struct_size = C.sizeof(_capi.PhotoLossArgs)
        a.channels, a.height, a.width = self.shape
        a.lambda_dssim, a.want_backward = lam, want_backward
        a.image, a.target, a.scratch, a.out = self.ptr("image"), self.ptr("target"), self.ptr("scratch"), self.ptr("out")
        a.dL_dloss, a.dL_dimage = self.ptr("up"), self.ptr("grad")
        a.stream = torch.cuda.current_stream().cuda_stream
        return a

    def read(self):
        """-> the buffer on the host; asserts that only scratch, out and grad differ from what was uploaded."""
        import torch
        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        same = _bits(got) == _bits(self.host)
        for name in ("scratch", "out", "grad"):
            same[self.slices[name]] = True
        assert same.all(), f"written outside scratch, out and dL_dimage at {np.nonzero(~same)[0][:8].tolist()}"
        return got


def _direct(x, y, lam, up, runs=1):
    """The two C calls on (x, y) in a fresh arena. -> (out f32[3] of every forward run, dL_dimage f32[C,H,W])"""
    from gsrast_amd import _capi
    L = _capi.lib()
    arena = _Arena(x, y, up)
    a = arena.args(lam)
    outs = []
    for _ in range(runs):
        _capi.check(L.gsr_photo_loss_forward(C.byref(a)), "gsr_photo_loss_forward")
        outs.append(arena.read()[arena.slices["out"]].copy())
    _capi.check(L.gsr_photo_loss_backward(C.byref(a)), "gsr_photo_loss_backward")
    got = arena.read()
    assert (_bits(got[arena.slices["out"]]) == _bits(outs[-1])).all()           # (the backward leaves the terms alone)
    return outs, got[arena.slices["grad"]].reshape(x.shape).copy()


def _within_an_ulp(got, want):
    want = np.float32(want)
    return got in (np.nextafter(want, np.float32(-np.inf)), want, np.nextafter(want, np.float32(np.inf)))


# ---- 1. the C entry points, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("up", UPS)
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_the_gradient_is_the_float32_restatement_bit_for_bit(shape, lam, up):
    x, y = _images(shape)
    want_grad, want_terms = _expected(shape, lam, up)
    outs, grad = _direct(x, y, lam, up, runs=2)
    assert (_bits(outs[0]) == _bits(outs[1])).all(), "out differs between two runs"
    for name, got, want in zip(("loss", "l1", "ssim"), outs[0], want_terms):
        print(f"[photo loss] {shape} lambda {lam} {name}: {got!r} (restatement {want!r})")
        assert _within_an_ulp(got, want), name
    differ = _bits(grad) != _bits(want_grad)
    assert not differ.any(), f"{int(differ.sum())} of {differ.size} floats differ, first at {np.argwhere(differ)[:4].tolist()}"
    if lam > 0 or (x != y).any():
        assert (want_grad != 0).any()


def test_a_forward_that_no_backward_follows_gives_the_same_terms():
    from gsrast_amd import _capi
    shape = (3, 33, 65)
    x, y = _images(shape)
    arena = _Arena(x, y, 1.0)
    _capi.check(_capi.lib().gsr_photo_loss_forward(C.byref(arena.args(0.2, want_backward=0))), "gsr_photo_loss_forward")
    out = arena.read()[arena.slices["out"]]
    assert (_bits(out) == _bits(_direct(x, y, 0.2, 1.0)[0][0])).all()


# ---- 2. photometric_loss --------------------------------------------------------------------------------------------------
def _cuda(a, requires_grad=False):
    import torch
    return torch.from_numpy(np.array(a)).cuda().requires_grad_(requires_grad)


@pytest.mark.parametrize("up", UPS)
def test_photometric_loss_is_the_direct_calls(up):
    import torch
    from gsrast_amd.loss import photometric_loss
    shape, lam = (3, 33, 65), 0.2
    x, y = _images(shape)
    outs, want_grad = _direct(x, y, lam, up)
    image, target = _cuda(x, True), _cuda(y)
    loss, l1, ssim = photometric_loss(image, target, return_terms=True)
    assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and loss.requires_grad
    assert not l1.requires_grad and not ssim.requires_grad and l1.shape == () and ssim.shape == ()
    (loss if up == 1.0 else up * loss).backward()
    torch.cuda.synchronize()
    got = np.array([loss.item(), l1.item(), ssim.item()], np.float32)
    assert (_bits(got) == _bits(outs[0])).all()
    assert image.grad.shape == image.shape and (_bits(image.grad.cpu().numpy()) == _bits(want_grad)).all()
    assert target.grad is None
    alone = photometric_loss(image, target, lambda_dssim=lam)                   # (without return_terms: the loss alone)
    assert isinstance(alone, torch.Tensor) and (_bits(np.float32(alone.item())) == _bits(outs[0][0])).all()


def test_an_image_without_requires_grad_gets_no_gradient():
    import torch
    from gsrast_amd.loss import photometric_loss
    shape = (3, 33, 65)
    x, y = _images(shape)
    image, target = _cuda(x), _cuda(y)
    loss = photometric_loss(image, target)
    assert not loss.requires_grad and loss.grad_fn is None and image.grad is None
    assert (_bits(np.float32(loss.item())) == _bits(_direct(x, y, 0.2, 1.0)[0][0][0])).all()
    with torch.no_grad():                                                       # the same inside no_grad, for a leaf that has one
        quiet = photometric_loss(_cuda(x, True), target)
    assert not quiet.requires_grad and quiet.item() == loss.item()


def test_a_view_offset_by_one_float_is_copied():
    import torch
    from gsrast_amd.loss import photometric_loss
    shape = (3, 33, 65)
    x, y = _images(shape)
    _, want_grad = _direct(x, y, 0.2, 1.0)
    base = torch.zeros(x.size + 1, device="cuda").requires_grad_(True)
    with torch.no_grad():
        base[1:] = _cuda(x.reshape(-1))
    view = base[1:].view(shape)
    tbase = torch.zeros(y.size + 1, device="cuda")
    tbase[1:] = _cuda(y.reshape(-1))
    assert view.data_ptr() % 16 == 4 and tbase[1:].data_ptr() % 16 == 4
    photometric_loss(view, tbase[1:].view(shape)).backward()
    torch.cuda.synchronize()
    got = base.grad.cpu().numpy()
    assert got[0] == 0 and (_bits(got[1:].reshape(shape)) == _bits(want_grad)).all()
    # ... and a transposed view
    flipped = _cuda(np.ascontiguousarray(x.transpose(0, 2, 1)), True)
    photometric_loss(flipped.transpose(1, 2), _cuda(y)).backward()
    assert (_bits(flipped.grad.transpose(1, 2).cpu().numpy()) == _bits(want_grad)).all()


def test_two_graphs_alive_at_once_share_nothing():
    import torch
    from gsrast_amd.loss import photometric_loss
    (xa, ya), (xb, yb) = _images((3, 33, 65)), _images((3, 11, 11))
    xc = np.ascontiguousarray(xa[:, ::-1, :])                                   # (a third, of the first one's shape)
    a, b, c = _cuda(xa, True), _cuda(xb, True), _cuda(xc, True)
    la, lb, lc = photometric_loss(a, _cuda(ya)), photometric_loss(b, _cuda(yb), 1.0), photometric_loss(c, _cuda(ya))
    lc.backward()
    la.backward()
    lb.backward()
    torch.cuda.synchronize()
    for image, x, y, lam, loss in ((a, xa, ya, 0.2, la), (b, xb, yb, 1.0, lb), (c, xc, ya, 0.2, lc)):
        outs, want = _direct(x, y, lam, 1.0)
        assert (_bits(np.float32(loss.item())) == _bits(outs[0][0])).all()
        assert (_bits(image.grad.cpu().numpy()) == _bits(want)).all()
    assert a.grad.data_ptr() != c.grad.data_ptr()


def test_photometric_loss_refuses_what_the_kernels_cannot_take():
    import torch
    from gsrast_amd.loss import photometric_loss
    x, y = _images((3, 7, 5))
    image, target = _cuda(x, True), _cuda(y)
    with pytest.raises(ValueError, match="not float32"):
        photometric_loss(image.double(), target)
    with pytest.raises(ValueError, match="not float32"):
        photometric_loss(image, target.half())
    with pytest.raises(ValueError, match=r"not \[C,H,W\]"):
        photometric_loss(image[0], target[0])
    with pytest.raises(ValueError, match=r"not \[C,H,W\]"):
        photometric_loss(image[None], target[None])
    with pytest.raises(ValueError, match="not on a GPU"):
        photometric_loss(image, target.cpu())
    with pytest.raises(ValueError, match="not on a GPU"):
        photometric_loss(image.detach().cpu(), target)
    with pytest.raises(ValueError, match="target"):
        photometric_loss(image, target[:, :6])
    for lam in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="lambda_dssim"):
            photometric_loss(image, target, lambda_dssim=lam)
    torch.cuda.synchronize()
    assert image.grad is None


# ---- 3. at the end of a rendered frame ------------------------------------------------------------------------------------
def test_the_loss_of_a_rendered_frame_reaches_the_parameters_and_the_optimiser_steps():
    """render() -> photometric_loss -> backward() fills params.*.grad with exactly what color.backward(gradient=G) gives for
    G the direct call's dL_dimage on the same colour image; GaussianAdam.step(radii) then moves the visible Gaussians."""
    import torch
    import step_frames as S
    from gsrast_amd.autograd import GaussianParams, RadiiSlot, render
    from gsrast_amd.loss import photometric_loss
    from gsrast_amd.optim import GaussianAdam
    from gsrast_amd.rasterizer import SplatRasterizer
    case = "gscuda"
    profile, deg, _, mod, _, _ = S.CASES[case]
    raw, cam = S.raw_scene(profile), S.camera_of(case)
    make = lambda: GaussianParams.from_raw(*(raw[k] for k in S.RAW), sh_layout="file", device="cuda:0")
    draw = dict(semantics=profile, sh_degree=deg, scale_modifier=mod, plan="sort", tile_history=False)
    rng = np.random.default_rng(3)
    target_np = rng.random((3, S.H, S.W)).astype(np.float32)
    target = _cuda(target_np)
    # through the loss
    params, slot = make(), RadiiSlot()
    color = render(params, SplatRasterizer(S.W, S.H, background=S.BG), cam, radii_slot=slot, **draw)[0]
    loss = photometric_loss(color, target)
    loss.backward()
    # the same frame, fed the direct call's gradient
    twin = make()
    color2 = render(twin, SplatRasterizer(S.W, S.H, background=S.BG), cam, **draw)[0]
    torch.cuda.synchronize()
    color_np = color2.detach().cpu().numpy()
    assert (_bits(color_np) == _bits(color.detach().cpu().numpy())).all()
    outs, G = _direct(color_np, target_np, 0.2, 1.0)
    assert (_bits(np.float32(loss.item())) == _bits(outs[0][0])).all()
    color2.backward(gradient=_cuda(G))
    torch.cuda.synchronize()
    for k in S.RAW:
        got, want = getattr(params, k).grad, getattr(twin, k).grad
        assert got is not None and bool((got != 0).any()), k
        assert (_bits(got.cpu().numpy()) == _bits(want.cpu().numpy())).all(), k
    before = {k: getattr(params, k).detach().clone() for k in S.RAW}
    opt = GaussianAdam(params.parameters(), lr=1e-3)
    opt.step(slot.radii)
    torch.cuda.synchronize()
    seen = (slot.radii > 0)
    assert bool(seen.any()) and not bool(seen.all())
    for k in S.RAW:
        moved = (getattr(params, k).detach() != before[k]).reshape(S.N, -1).any(1)
        assert bool(moved.any()) and not bool(moved[~seen].any()), k
