"""GPU: the error contract (include/gsrast_amd.h) of the entry points whose every success is a launch — after another
entry point was refused, one valid call on real device memory returns GSR_OK and leaves GSR_OK as the last error, with no
HIP text. The smallest shapes that launch every kernel of the call: 64 Gaussians, a 3 x 16 x 64 image, a 64 x 64 frame.
What the kernels compute is pinned by their own suites; tests/test_capi_cpu.py holds the rows that need no device."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, W, H = 64, 64, 64


def _refuse_another(L):
    """gsr_forward with null fields: refused before anything is launched, and recorded."""
    from gsrast_amd import _capi
    a = _capi.ForwardArgs(struct_size=C.sizeof(_capi.ForwardArgs))
    assert L.gsr_forward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG and L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG


def _params():
    from gsrast_amd.autograd import GaussianParams
    rng = np.random.default_rng(7)
    rotation = np.tile(np.float32([1, 0, 0, 0]), (N, 1)) + 0.1 * rng.normal(size=(N, 4)).astype(np.float32)
    return GaussianParams.from_raw(rng.uniform(-0.5, 0.5, (N, 3)), np.full(N, 1.0), np.full((N, 3), np.log(0.1)), rotation,
                                   0.3 * rng.normal(size=(N, 48)), device="cuda:0")


def _drawn():
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    rast = SplatRasterizer(W, H, device="cuda:0")
    rast.configure_from_scene(scenes.isotropic_scene(N, 42))
    rast.draw(camera.default_camera(W, H))
    assert rast.last_num_rendered > 0
    return rast


def _new(*shape, dtype=None, fill=None):
    import torch
    t = torch.zeros(shape, dtype=dtype or torch.float32, device="cuda:0")
    return t if fill is None else t.fill_(fill)


# Each case prepares, calls refuse() and then makes its ONE status-returning call (the Python wrappers raise unless it returns
# GSR_OK; between refuse() and that call they make no other). A rasterizer is returned: giving it up is a call of its own
# (gsr_tile_history_destroy), which must not come before the test has looked.
def _activate_params(L, refuse):
    p = _params()
    refuse()
    p.activated()


def _activate_params_backward(L, refuse):
    # (called here, not through loss.backward(): autograd runs a backward on a thread of its own, and the last error is the
    # calling thread's)
    from gsrast_amd import _capi
    p = _params()
    ups = [_new(N, 4, fill=1.0) for _ in range(4)]                  # dL_dmeans3D, dL_dscales, dL_drotations, dL_dconic_opacity
    outs = [_new(N, 3), _new(N), _new(N, 3), _new(N, 4)]
    refuse()
    _capi.call("gsr_activate_params_backward", N, p.opacity_logit.data_ptr(), p.log_scale.data_ptr(), p.rotation.data_ptr(), None,
               *(t.data_ptr() for t in ups + outs), _capi.stream(ups[0].device), device=ups[0].device)


def _ply_activate_layout(L, refuse):
    from gsrast_amd import _capi
    raw, out = _new(N * 62, fill=0.5), [_new(N, 4), _new(N, 4), _new(N, 4), _new(N), _new(N, 48)]
    refuse()
    _capi.call("gsr_ply_activate_layout", raw.data_ptr(), N, *(t.data_ptr() for t in out), _capi.GSR_SH_LAYOUT_COEFFICIENT_MAJOR,
               _capi.stream(raw.device), device=raw.device)


def _photo_loss(backward):
    def case(L, refuse):
        import torch
        from gsrast_amd import _capi
        image, target, out, up, grad = _new(3, 16, 64, fill=0.25), _new(3, 16, 64, fill=0.5), _new(3), _new(1, fill=1.0), _new(3, 16, 64)
        scratch = _new(int(L.gsr_photo_loss_scratch_bytes(3, 64, 16)), dtype=torch.uint8)
        a = _capi.PhotoLossArgs(struct_size=C.sizeof(_capi.PhotoLossArgs), channels=3, width=64, height=16, lambda_dssim=0.2,
                                image=image.data_ptr(), target=target.data_ptr(), scratch=scratch.data_ptr(), out=out.data_ptr(),
                                dL_dloss=up.data_ptr(), dL_dimage=grad.data_ptr(), want_backward=1, stream=_capi.stream(image.device))
        if not backward:
            refuse()
        _capi.call("gsr_photo_loss_forward", C.byref(a), device=image.device)
        if backward:                                                # (here, not through loss.backward(): see above)
            refuse()
            _capi.call("gsr_photo_loss_backward", C.byref(a), device=image.device)
    return case


def _densify_plan(L, refuse):
    import torch
    from gsrast_amd import _capi
    from gsrast_amd.densify import plan_scalars
    i32 = torch.int32
    temp = _new(int(L.gsr_densify_plan_temp_bytes(N)), dtype=torch.uint8)
    arrays = [_new(N, fill=1.0), _new(N, 3, fill=-2.0), _new(N, fill=1e-3), _new(N, dtype=i32, fill=2), _new(N, dtype=i32, fill=5)]
    src_of, counts = _new(3 * N, dtype=i32), _new(4, dtype=i32)
    refuse()
    _capi.call("gsr_densify_plan", N, *(t.data_ptr() for t in arrays), *plan_scalars(2e-4, 0.005, 1.0, 0.01), 0, temp.data_ptr(),
               src_of.data_ptr(), counts.data_ptr(), _capi.stream(temp.device), device=temp.device)
    assert counts.tolist()[3] > 0                                   # (all three kernels had rows to work on)


def _adam_step(L, refuse):
    import torch
    from gsrast_amd.optim import GaussianAdam
    p = _params()
    for t in p.parameters():
        t.grad = torch.ones_like(t)
    opt = GaussianAdam(list(p.parameters()), lr=1e-3)
    refuse()
    opt.step()


def _densify_accumulate(L, refuse):
    import torch
    from gsrast_amd.autograd import FrameSlot
    from gsrast_amd.densify import DensityStats
    stats, slot = DensityStats(N, "cuda:0"), FrameSlot()
    slot.radii, slot.dL_dmean2D = _new(N, dtype=torch.int32, fill=3), _new(N, 2, fill=1e-3)
    refuse()
    stats.update(slot, W, H)


def _densify_apply(L, refuse):
    import torch
    from gsrast_amd import _capi
    a = _capi.DensifyApplyArgs()
    a.struct_size, a.n_src = C.sizeof(_capi.DensifyApplyArgs), N
    a.counts[:] = [N, 0, 0, N]                                      # every row kept, in place
    src_of = torch.arange(N, dtype=torch.int32, device="cuda:0")
    a.src_of, a.stream = src_of.data_ptr(), _capi.stream(src_of.device)
    keep = []
    for k, cols in (("xyz", 3), ("opacity_logit", 1), ("log_scale", 3), ("rotation", 4), ("shs", 48)):
        keep += [_new(N, cols, fill=0.5), _new(N, cols)]
        getattr(a, k).src, getattr(a, k).dst = keep[-2].data_ptr(), keep[-1].data_ptr()
    refuse()
    _capi.call("gsr_densify_apply", C.byref(a), device=src_of.device)


def _backward(L, refuse):
    rast = _drawn()
    refuse()
    rast.backward(_new(3, H, W, fill=1.0))
    return rast


def _camera_backward(L, refuse):
    rast = _drawn()
    grads = rast.backward(_new(3, H, W, fill=1.0))
    refuse()
    rast.camera_backward(grads)
    return rast


def _forward_points(L, refuse):
    rast = _drawn()
    refuse()
    rast.draw_points()
    return rast


CASES = {"gsr_activate_params": _activate_params, "gsr_activate_params_backward": _activate_params_backward,
         "gsr_ply_activate_layout": _ply_activate_layout, "gsr_photo_loss_forward": _photo_loss(False),
         "gsr_photo_loss_backward": _photo_loss(True), "gsr_densify_plan": _densify_plan, "gsr_adam_step": _adam_step,
         "gsr_densify_accumulate": _densify_accumulate, "gsr_densify_apply": _densify_apply, "gsr_backward": _backward,
         "gsr_camera_backward": _camera_backward, "gsr_forward_points": _forward_points}


@pytest.mark.parametrize("name", list(CASES))
def test_a_launching_call_after_a_refusal_leaves_no_error(name):
    import torch
    from gsrast_amd import _capi
    L = _capi.lib()
    refused = []
    alive = CASES[name](L, lambda: refused.append(_refuse_another(L)))
    assert len(refused) == 1
    assert L.gsr_last_error() == _capi.GSR_OK and L.gsr_last_hip_error() == b"", name
    torch.cuda.synchronize()
    del alive
