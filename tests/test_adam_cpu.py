"""CPU: the references of the Adam step (tests/adam_ref.py) against torch.optim.Adam and against each other, what a culled
row means in them, and every refusal of gsr_adam_step and of gsrast_amd.optim.GaussianAdam that needs no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import adam_ref as R
from helpers import ROOT

from gsrast_amd import _capi
from gsrast_amd.optim import GaussianAdam, adam_scalars


# ---- 1. step32 against torch and float64 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [1e-8, 1e-15])
def test_step32_is_as_close_to_float64_as_torchs_adam(eps):
    """Five steps over 200 000 values, gradients a normal draw times 10^U(-6, 1) (a magnitude per value, a fresh draw per
    step). step32 and torch.optim.Adam(foreach=False) on the CPU are two float32 roundings of the same formula: each is
    compared with step64, and step32's largest error — absolute for p, relative for m and v — is at most twice torch's."""
    n, steps, lr = 200_000, 5, 1e-2
    rng = np.random.default_rng(20)
    p0 = rng.normal(size=n).astype(np.float32)
    mag = 10.0 ** rng.uniform(-6, 1, n)
    grads = [(rng.normal(size=n) * mag).astype(np.float32) for _ in range(steps)]
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, eps=eps, foreach=False)
    p32, m32, v32 = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    p64, m64, v64 = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads, 1):
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        p32, m32, v32 = R.step32(p32, g, m32, v32, t, lr=lr, eps=eps)
        p64, m64, v64 = R.step64(p64, g, m64, v64, t, lr=lr, eps=eps)
    st = opt.state[tp]
    torchs = (tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy())
    assert int(st["step"]) == steps
    moved = float(np.abs(p64 - p0).max())
    print(f"[adam ref] eps={eps:g}: parameters moved by up to {moved:.4f}")
    assert moved > 1e-2                                              # (a test of nothing otherwise)
    assert (m64 != 0).all() and (v64 > 0).all()
    for name, ours, theirs, want, relative in (("p", p32, torchs[0], p64, False), ("exp_avg", m32, torchs[1], m64, True),
                                               ("exp_avg_sq", v32, torchs[2], v64, True)):
        scale = np.abs(want) if relative else 1.0
        e_ours = float((np.abs(ours.astype(np.float64) - want) / scale).max())
        e_torch = float((np.abs(theirs.astype(np.float64) - want) / scale).max())
        print(f"[adam ref] eps={eps:g} {name}: step32 {e_ours:.3e}, torch {e_torch:.3e} ({'relative' if relative else 'absolute'})")
        assert e_torch > 0 and e_ours <= 2.0 * e_torch, name


def test_the_hosts_scalars_are_the_references():
    """optim.adam_scalars (doubles, rounded by ctypes on assignment) and adam_ref.scalars32 (np.float32 of the doubles)."""
    for t in (1, 2, 7, 1001, 30000):
        for lr, b1, b2, eps in ((1e-3, 0.9, 0.999, 1e-8), (1.6e-4, 0.9, 0.999, 1e-15), (2.5e-2, 0.8, 0.99, 1e-6)):
            slot = _capi.AdamTensor()
            slot.step_size, slot.rs, slot.b1c, slot.b2, slot.b2c, slot.eps = adam_scalars(lr, b1, b2, eps, t)
            got = np.array([slot.step_size, slot.rs, slot.b1c, slot.b2, slot.b2c, slot.eps], np.float32)
            assert (got.view(np.uint32) == np.array(R.scalars32(lr, b1, b2, eps, t), np.float32).view(np.uint32)).all()


# ---- 2. what a culled row means ---------------------------------------------------------------------------------------------
def test_culled_rows_keep_their_bits_and_the_step_count_advances_without_them():
    rng = np.random.default_rng(21)
    n, w = 40, 3
    p0 = rng.normal(size=(n, w)).astype(np.float32)
    m0 = (0.1 * rng.normal(size=(n, w))).astype(np.float32)
    v0 = (0.01 * rng.uniform(0.1, 1, (n, w))).astype(np.float32)
    g = rng.normal(size=(n, w)).astype(np.float32)
    visible = rng.integers(-2, 3, n).astype(np.int32)                # negative, zero and positive
    assert (visible < 0).any() and (visible == 0).any() and (visible > 0).any()
    off = visible <= 0
    g_nan = g.copy()
    g_nan[off] = np.nan
    bits = lambda a: a.view(np.uint32)
    for ref in (R.step32, R.step64):
        p1, m1, v1 = ref(p0, g_nan, m0, v0, 4, visible=visible)
        dense = ref(p0, g, m0, v0, 4)
        for new, old, full in zip((p1, m1, v1), (p0, m0, v0), dense):
            old = old.astype(new.dtype)
            assert (new[off].view(np.uint8) == old[off].view(np.uint8)).all()           # bit for bit, the gradient never read
            assert np.array_equal(new[~off], full[~off]) and (new[~off] != old[~off]).any()
    # the bias correction is by the global count: rows seen at steps 1 and 3 only get step 3's scalars at step 3
    seen = (visible > 0).astype(np.int32)
    g2, g3 = (rng.normal(size=(n, w)).astype(np.float32) for _ in range(2))
    a = R.step32(p0, g, m0, v0, 1)
    b = R.step32(a[0], g2, a[1], a[2], 2, visible=1 - seen)          # step 2 sees the others
    c = R.step32(b[0], g3, b[1], b[2], 3, visible=seen)
    want = R.step32(a[0], g3, a[1], a[2], 3)                         # for the rows step 2 skipped: as if it had not happened, t = 3
    wrong = R.step32(a[0], g3, a[1], a[2], 2)                        # ... and not their own second update
    on = seen > 0
    for x, y in zip(c, want):
        assert (bits(x[on]) == bits(y[on])).all()
    assert (bits(c[0][on]) != bits(wrong[0][on])).any()


# ---- 3. the C ABI's refusals ------------------------------------------------------------------------------------------------
def _args(n_tensors=2, rows=10):
    """Arguments gsr_adam_step accepts, with made-up 16-byte-aligned addresses (no test here lets the call reach a launch)."""
    a = _capi.AdamArgs()
    a.struct_size, a.num_tensors, a.num_rows = C.sizeof(_capi.AdamArgs), n_tensors, rows
    for k in range(n_tensors):
        t = a.tensors[k]
        t.param, t.grad, t.exp_avg, t.exp_avg_sq = (0x10000 * (4 * k + j + 1) for j in range(4))
        t.row_floats = (3, 48)[k % 2]
        t.step_size, t.rs, t.b1c, t.b2, t.b2c, t.eps = adam_scalars(1e-3, 0.9, 0.999, 1e-8, 1)
    return a


def test_adam_step_refuses_bad_arguments_before_any_hip_call():
    L = _capi.lib()
    bad = _capi.GSR_ERR_INVALID_ARG
    call = lambda a: L.gsr_adam_step(C.byref(a))
    assert L.gsr_adam_step(None) == bad
    a = _args()
    a.num_rows = 0
    assert call(a) == _capi.GSR_OK                                   # the arguments of every refusal below are otherwise these
    for size in (0, C.sizeof(_capi.AdamArgs) - 8, C.sizeof(_capi.AdamArgs) + 8):
        a = _args()
        a.struct_size = size
        assert call(a) == bad, size
    for count in (-1, 0, _capi.GSR_ADAM_MAX_TENSORS + 1):
        a = _args()
        a.num_tensors = count
        assert call(a) == bad, count
    a = _args()
    a.num_rows = -1
    assert call(a) == bad
    for k in (0, 1):
        for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
            a = _args()
            setattr(a.tensors[k], field, None)
            assert call(a) == bad, (k, field, "null")
            for off in (4, 8, 12, 1):
                a = _args()
                setattr(a.tensors[k], field, getattr(a.tensors[k], field) + off)
                assert call(a) == bad, (k, field, off)
        for rf in (0, -1, -48):
            a = _args()
            a.tensors[k].row_floats = rf
            assert call(a) == bad, (k, rf)
    # ... also with no rows to update, and the thread's last error says so
    a = _args()
    a.num_rows = 0
    a.tensors[1].grad = None
    assert call(a) == bad and L.gsr_last_error() == bad
    # a tensor past num_tensors is not looked at
    a = _args(n_tensors=1)
    a.num_rows = 0
    assert call(a) == _capi.GSR_OK


def test_adam_args_have_the_headers_layout(tmp_path):
    """The header compiled as C prints sizes and offsets: the ctypes mirrors agree field for field."""
    probes = {"gsr_adam_tensor": (_capi.AdamTensor, [f for f, _ in _capi.AdamTensor._fields_]),
              "gsr_adam_args": (_capi.AdamArgs, [f for f, _ in _capi.AdamArgs._fields_])}
    lines = []
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    lines.append('printf("max %d\\n", GSR_ADAM_MAX_TENSORS);')
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + "".join(lines) + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    assert int(got["max"]) == _capi.GSR_ADAM_MAX_TENSORS == 8
    for cname, (ctype, fields) in probes.items():
        assert int(got[cname]) == C.sizeof(ctype), cname
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(ctype, f).offset, f"{cname}.{f}"


# ---- 4. the optimiser's refusals --------------------------------------------------------------------------------------------
def _with_grad(t, grad=None):
    p = torch.nn.Parameter(t)
    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format) if grad is None else grad
    return p


def _off_by_a_float(shape):
    """A contiguous tensor that starts four bytes past a 16-byte boundary."""
    n = int(np.prod(shape))
    t = torch.zeros(n + 4)[1:n + 1].reshape(shape)
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def test_gaussian_adam_refuses_what_the_kernel_cannot_take():
    ok = lambda: torch.zeros(8, 3)
    cases = {}
    cases["not on a GPU"] = _with_grad(ok())                                         # a CPU parameter, fine otherwise
    cases["not float32"] = _with_grad(torch.zeros(8, 3, dtype=torch.float64))
    cases["a parameter is not contiguous"] = _with_grad(torch.zeros(8, 6)[:, :3])
    cases["a parameter does not start on a 16-byte boundary"] = _with_grad(_off_by_a_float((8, 3)))
    cases["a gradient does not start on a 16-byte boundary"] = _with_grad(ok(), _off_by_a_float((8, 3)))
    cases["a gradient is not contiguous"] = _with_grad(ok(), torch.zeros(3, 8).t())
    cases["a gradient is sparse"] = _with_grad(ok(), torch.zeros(8, 3).to_sparse())
    other = _with_grad(ok())
    other.grad.data = torch.zeros(9, 3)                                              # (assigning .grad itself checks the shape)
    cases["a gradient is (9, 3)"] = other
    for message, p in cases.items():
        opt = GaussianAdam([p])
        with pytest.raises(ValueError, match=message.replace("(", r"\(").replace(")", r"\)")):
            opt.step()
        assert len(opt.state[p]) == 0, message                                       # nothing was begun
    # state a trainer put there
    for key in ("exp_avg", "exp_avg_sq"):
        for message, t in ((f"state {key} does not start on a 16-byte boundary", _off_by_a_float((8, 3))),
                           (f"state {key} is not contiguous", torch.zeros(3, 8).t()),
                           (f"state {key} is \\(7, 3\\)", torch.zeros(7, 3)),
                           (f"state {key} is torch.float64", torch.zeros(8, 3, dtype=torch.float64))):
            p = _with_grad(ok())
            opt = GaussianAdam([p])
            opt.state[p].update(step=3, exp_avg=torch.zeros(8, 3), exp_avg_sq=torch.zeros(8, 3))
            opt.state[p][key] = t
            with pytest.raises(ValueError, match=message):
                opt.step()
            assert opt.state[p]["step"] == 3
    # a parameter without a gradient is skipped entirely: no refusal, no state
    p = torch.nn.Parameter(torch.zeros(8, 3, dtype=torch.float64))
    opt = GaussianAdam([p])
    opt.step()
    assert len(opt.state[p]) == 0
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1))):
        with pytest.raises(ValueError):
            GaussianAdam([torch.nn.Parameter(ok())], **kw)
    opt = GaussianAdam([torch.nn.Parameter(ok())])
    assert all(opt.defaults[k] == v for k, v in dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8).items())      # torch's Adam defaults
