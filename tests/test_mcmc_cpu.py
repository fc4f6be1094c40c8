"""CPU: the reference of the 3DGS-MCMC calls (tests/mcmc_ref.py) against the paper's two conditions and against float64;
gsrast_amd.mcmc.sample_rows; the C ABI's fourth table (_capi.MCMC_SIGNATURES, include/gsrast_amd_mcmc.h) held to the same
contract tests as the others; every refusal of the three calls. No GPU call is made."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mcmc_ref as R
from helpers import ROOT

from gsrast_amd import _capi, mcmc

F = np.float32
RATIOS = (1, 2, 3, 10, 51)
OPACITIES = (0.006, 0.1, 0.5, 0.99)


# ---- the relocation against the paper's two conditions, in float64 ----
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("o", OPACITIES)
def test_relocated_opacity_composites_to_the_old_one(o, ratio):
    """ratio copies of opacity o_new on top of each other are as opaque as the one before: 1 - (1 - o_new)^ratio == o."""
    o_new, _, _, _ = R.relocated(F(o), ratio, F(1e-6))
    assert abs((1.0 - (1.0 - o_new) ** ratio) - float(F(o))) <= 1e-12


def _trapezoid(f, half_width, steps):
    x = np.linspace(-half_width, half_width, steps + 1)
    y = f(x)
    return float((y.sum() - 0.5 * (y[0] + y[-1])) * (x[1] - x[0]))


@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("o", OPACITIES)
def test_relocated_scale_keeps_the_integral(o, ratio):
    """The paper's second condition along a line through the centre: ratio copies of (o_new, s') cover what (o, s) covered,
      int 1 - (1 - o_new exp(-x^2 / 2 s'^2))^ratio dx == int o exp(-x^2 / 2 s^2) dx = o s sqrt(2 pi),     s' = s o / D.
    Quadrature: the trapezoid rule over +-14 of the wider standard deviation, which converges geometrically for a Gaussian
    integrand; its own error is shown by halving the step (the two results agree to 1e-13 of the value, and the tails beyond
    14 sigma are below exp(-98)); the bound used is 1e-10 of the value."""
    o32 = float(F(o))
    o_new, D, _, shift = R.relocated(F(o), ratio, F(1e-6))
    s = 0.37
    s_new = s * o32 / D
    assert abs(np.log(s_new / s) - shift) <= 1e-14                           # (the shift IS log(o / D))
    f = lambda x: 1.0 - (1.0 - o_new * np.exp(-x * x / (2.0 * s_new * s_new))) ** ratio
    half = 14.0 * max(s, s_new)
    coarse, fine = _trapezoid(f, half, 20000), _trapezoid(f, half, 40000)
    want = o32 * s * np.sqrt(2.0 * np.pi)
    assert abs(coarse - fine) <= 1e-13 * want, "the quadrature itself"
    print(f"o {o} ratio {ratio}: o_new {o_new:.6g} D {D:.6g} integral off by {abs(fine - want) / want:.2e}")
    assert abs(fine - want) <= 1e-10 * want


@pytest.mark.parametrize("o", OPACITIES)
def test_a_ratio_of_one_changes_nothing(o):
    o_new, D, logit, shift = R.relocated(F(o), 1, F(1e-6))
    o32 = float(F(o))
    assert abs(o_new - o32) <= 4e-16 and D == o_new and abs(shift) <= 1e-15
    assert abs(logit - np.log(o32 / (1.0 - o32))) <= 1e-13


def test_relocation_clamps():
    """o = 1.0f (opacity_logit = 30): finite, clamped to 1 - 2^-23; and a new opacity below min_opacity is lifted to it."""
    o_new, D, logit, shift = R.relocated(F(1.0), 2, F(0.005))
    assert o_new == 1.0 and np.isfinite([D, logit, shift]).all()
    assert logit == np.log(R.TOP / (1.0 - R.TOP))
    _, _, logit, _ = R.relocated(F(0.006), 51, F(0.005))
    m = float(F(0.005))
    assert logit == np.log(m / (1.0 - m))


def test_relocate_steps_by_hand():
    """Five rows; row 1 drawn twice, row 3 once, one index out of range: the multiplicities, the rows touched, the copies."""
    n = 5
    rng = np.random.default_rng(0)
    raw = {k: rng.normal(size=(n, R.WIDTHS[k]) if k != "opacity_logit" else n).astype(F) for k in R.RAW}
    moments = {k: (np.ones_like(raw[k]), np.ones_like(raw[k])) for k in R.RAW}
    o = (1.0 / (1.0 + np.exp(-raw["opacity_logit"].astype(np.float64)))).astype(F)
    out = R.relocate(raw, moments, [1, 3, 7, 1], [0, 2, 4, 4], F(0.005), o)
    assert out["rejected"] == 1 and out["counts"].tolist() == [0, 2, 0, 1, 0]
    for k in R.RAW:
        got = out["raw"][k].reshape(n, -1)
        assert (got[0] == got[1]).all() and (got[4] == got[1]).all() and (got[2] == got[3]).all(), k
        m, v = (a.reshape(n, -1) for a in out["moments"][k])
        assert not m.any() and not v.any()                                  # rows 1, 3 (sources) and 0, 2, 4 (destinations): all five
        if k not in ("opacity_logit", "log_scale"):
            assert (got[1] == raw[k].reshape(n, -1)[1]).all()
    assert out["raw"]["opacity_logit"][1] < raw["opacity_logit"][1] and (out["raw"]["log_scale"][1] < raw["log_scale"][1]).all()
    none = R.relocate(raw, {}, [1], None, F(0.005), o)                       # no destinations: the source alone changes
    same = [i for i in range(n) if i != 1]
    for k in R.RAW:
        assert (none["raw"][k][same] == raw[k][same]).all()


# ---- the noise against float64 ----
def _noise_case(n=4000, seed=3):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F)
    s = rng.uniform(0.5, 2.0, (n, 3)).astype(F)
    v = rng.normal(size=(n, 3)).astype(F)
    return v, s, q


def _sigma_v(v, s, q):
    Rm = R.build_rotation(q.astype(np.float64))
    S2 = s.astype(np.float64) ** 2
    return np.einsum("naj,nj,nbj,nb->na", Rm, S2, Rm, v.astype(np.float64))


def _noise_bound(v, s):
    """|float32 result - float64 result| per component. Every entry of R carries at most 4 roundings on values of at most 2,
    every one of the 18 products and 12 additions one more, the two scalings one each; each partial result is at most
    smax^2 |v|_1 in magnitude (|R_ij| <= 1 up to rounding): 3 terms x (4 + 4 + 2 + 2) roundings, doubled for the second
    rotation's inputs carrying the first's error: 72 u smax^2 |v|_1 with u = 2^-24."""
    return 72.0 * 2.0 ** -24 * (s.astype(np.float64).max(axis=1) ** 2 * np.abs(v.astype(np.float64)).sum(axis=1))[:, None]


def test_noise_reference_is_sigma_times_v():
    v, s, q = _noise_case()
    got = R.noise_move(v, s, q)
    assert got.dtype == F
    err = np.abs(got.astype(np.float64) - _sigma_v(v, s, q))
    print(f"worst error / bound: {(err / _noise_bound(v, s)).max():.3f}")
    assert (err <= _noise_bound(v, s)).all()


@pytest.mark.parametrize("drop", [(stage, a, j) for stage in range(2) for a in range(3) for j in range(3)])
def test_noise_check_sees_a_dropped_product(drop):
    """The blindness guard: with any one of the nine products of either rotation left out, the check above fails — on most
    rows, in the component the product belongs to (every component, for a product of the first rotation)."""
    v, s, q = _noise_case()
    err = np.abs(R.noise_move(v, s, q, drop=drop).astype(np.float64) - _sigma_v(v, s, q))
    over = err > _noise_bound(v, s)
    assert (over[:, drop[1]] if drop[0] == 1 else over.any(axis=1)).mean() > 0.9


def test_noise_reference_gates_by_opacity():
    o = np.array([0.001, 0.005, 0.5, 0.999], F)
    t = R.gate_argument(o)
    assert t.dtype == F and t[0] > 0 and abs(t[1]) < 1e-4 and t[2] < -49 and t[3] < -99
    xyz = np.zeros((4, 3), F)
    z = np.ones((4, 3), F)
    q = np.tile(np.array([1, 0, 0, 0], F), (4, 1))
    g = (1.0 / (1.0 + np.exp(-t.astype(np.float64)))).astype(F)
    moved = R.noise(xyz, z, 1.0, np.ones((4, 3), F), q, g)
    assert (moved[0] > 0.59).all() and (moved[2] < 1e-20).all() and (moved[3] < 1e-40).all()
    assert (R.noise(xyz + F(1.5), z, 0.0, np.ones((4, 3), F), q, g) == F(1.5)).all()


# ---- sample_rows ----
def test_sample_rows_never_returns_a_row_of_weight_zero():
    w = torch.tensor([0.0, 0.0, 1.0, 0.0, 2.0, 0.5, 0.0, 0.0], dtype=torch.float32)
    cdf = np.cumsum(w.numpy().astype(np.float64))
    below_one = float(np.nextafter(1.0, 0.0))
    u = [0.0, below_one] + [c / cdf[-1] for c in cdf[:-1]] + [float(np.nextafter(c / cdf[-1], 0.0)) for c in cdf if c > 0]
    u = torch.tensor([x for x in u if x < 1.0], dtype=torch.float64)
    got = mcmc.sample_rows(w, u)
    assert got.dtype == torch.int64 and (w[got] > 0).all()
    assert got[0] == 2 and got[1] == 5
    assert got.tolist() == R.sample_rows(w.numpy(), u.numpy()).tolist()
    # a total whose product with the largest double below 1 rounds up to the total itself: the last row of non-zero weight
    w3 = torch.tensor([1.0, 2.0 ** -60, 0.0], dtype=torch.float64)
    assert float(torch.tensor(below_one, dtype=torch.float64) * w3.sum()) * (1 + 2.0 ** -52) >= float(w3.sum())
    for x in (below_one, 1.0 - 2.0 ** -30):
        assert w3[mcmc.sample_rows(w3, torch.tensor([x], dtype=torch.float64))] > 0
    tiny = torch.tensor([3.0, 0.0, 0.0])
    assert mcmc.sample_rows(tiny, torch.tensor([0.0, below_one], dtype=torch.float64)).tolist() == [0, 0]


def test_sample_rows_frequencies():
    w = torch.tensor([1.0, 0.0, 3.0, 6.0])
    draws = 200_000
    u = torch.rand(draws, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    freq = np.bincount(mcmc.sample_rows(w, u).numpy(), minlength=4) / draws
    p = w.numpy() / 10.0
    # five standard deviations of a binomial frequency
    assert (np.abs(freq - p) <= 5.0 * np.sqrt(p * (1 - p) / draws)).all() and freq[1] == 0


def test_sample_rows_takes_more_rows_than_multinomial():
    n = (1 << 24) + 1
    w = torch.ones(n, dtype=torch.float32)
    with pytest.raises(RuntimeError):
        torch.multinomial(w, 1)
    got = mcmc.sample_rows(w, torch.tensor([0.0, 0.5, float(np.nextafter(1.0, 0.0))], dtype=torch.float64))
    assert got.tolist() == [0, n // 2, n - 1]


def test_sample_rows_refuses_all_zero_weights():
    for w in (torch.zeros(5), torch.zeros(0)):
        with pytest.raises(ValueError, match="every weight is 0"):
            mcmc.sample_rows(w, torch.zeros(1, dtype=torch.float64))


# ---- the C ABI: the fourth table against its header, and the error contract of its status-returning calls ----
def _declared_functions():
    text = open(os.path.join(ROOT, "include", "gsrast_amd_mcmc.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_mcmc_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert len(names) == 5
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_mcmc.h but not exported"
    assert set(_capi.MCMC_SIGNATURES) == set(names), "ctypes table and header disagree"
    for other in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES):
        assert not set(_capi.MCMC_SIGNATURES) & set(other)


def test_python_constants_and_structs_are_the_mcmc_headers(tmp_path):
    import subprocess
    probes = {"GSR_MCMC_MAX_ROWS": _capi.GSR_MCMC_MAX_ROWS, "GSR_MCMC_MAX_RATIO": _capi.GSR_MCMC_MAX_RATIO,
              "sizeof(gsr_mcmc_noise_args)": C.sizeof(_capi.McmcNoiseArgs), "sizeof(gsr_mcmc_relocate_args)": C.sizeof(_capi.McmcRelocateArgs),
              "offsetof(gsr_mcmc_noise_args, noise)": _capi.McmcNoiseArgs.noise.offset,
              "offsetof(gsr_mcmc_relocate_args, shs)": _capi.McmcRelocateArgs.shs.offset,
              "offsetof(gsr_mcmc_relocate_args, temp)": _capi.McmcRelocateArgs.temp.offset}
    body = "".join(f'printf("%lld\\n", (long long)({k}));' for k in probes)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_mcmc.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [int(v) for v in probes.values()], dict(zip(probes, got))
    assert R.MAX_RATIO == _capi.GSR_MCMC_MAX_RATIO


_AT = 0x10000                                               # an invented, 16-byte aligned address: no call here dereferences it
_INVALID, _TOO_LARGE = _capi.GSR_ERR_INVALID_ARG, _capi.GSR_ERR_TOO_LARGE
_forward_nulls = lambda: (C.byref(_capi.ForwardArgs(struct_size=C.sizeof(_capi.ForwardArgs))),)


def _noise_args(n=5, **change):
    a = _capi.McmcNoiseArgs()
    a.struct_size, a.scaler, a.n = C.sizeof(_capi.McmcNoiseArgs), 1.0, n
    a.xyz = a.opacity_logit = a.log_scale = a.rotation = a.noise = _AT
    for k, v in change.items():
        setattr(a, k, v)
    return (C.byref(a),)


def _relocate_args(n=5, m=3, min_opacity=0.005, **change):
    a = _capi.McmcRelocateArgs()
    a.struct_size, a.min_opacity, a.n, a.m = C.sizeof(_capi.McmcRelocateArgs), min_opacity, n, m
    a.sampled = a.dst = a.temp = _AT
    for k in R.RAW:
        getattr(a, k).param = _AT
    for k, v in change.items():
        if "." in k:
            getattr(a, k.split(".")[0]).__setattr__(k.split(".")[1], v)
        else:
            setattr(a, k, v)
    return (C.byref(a),)


# name -> (arguments that are refused, the code, arguments of a success that makes no HIP call). No row reaches a HIP call.
MCMC_ERROR_CONTRACT = {
    "gsr_mcmc_noise": (lambda: _noise_args(struct_size=3), _INVALID, lambda: _noise_args(n=0)),
    "gsr_mcmc_plan": (lambda: (1, None, 0.0, None, None, None, None, None), _INVALID, None),     # (n == 0 clears the counts: a HIP call)
    "gsr_mcmc_relocate": (lambda: (None,), _INVALID, lambda: _relocate_args(m=0)),
}


def test_the_mcmc_error_contract_table_names_every_status_returning_entry_point():
    derived = {name for name, (res, _) in _capi.MCMC_SIGNATURES.items() if res is C.c_int}
    assert derived == set(MCMC_ERROR_CONTRACT), sorted(derived ^ set(MCMC_ERROR_CONTRACT))


@pytest.mark.parametrize("name", sorted(MCMC_ERROR_CONTRACT))
def test_every_status_returning_mcmc_entry_point_keeps_the_error_contract(name):
    """As tests/test_capi_cpu.py: a refusal returns its code and leaves it as the last error; a success returns GSR_OK and
    leaves GSR_OK, directly after another entry point was refused; neither leaves a HIP text."""
    L = _capi.lib()
    refused, code, fine = MCMC_ERROR_CONTRACT[name]
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert getattr(L, name)(*refused()) == code
    assert L.gsr_last_error() == code and L.gsr_last_hip_error() == b""
    if fine is not None:
        assert L.gsr_forward(*_forward_nulls()) == _INVALID and L.gsr_last_error() == _INVALID
        assert getattr(L, name)(*fine()) == _capi.GSR_OK
        assert L.gsr_last_error() == _capi.GSR_OK and L.gsr_last_hip_error() == b""


_BIG = _capi.GSR_MCMC_MAX_ROWS + 1
_REFUSALS = [
    ("gsr_mcmc_noise", lambda: (None,), _INVALID),
    ("gsr_mcmc_noise", lambda: _noise_args(struct_size=C.sizeof(_capi.McmcNoiseArgs) + 8), _INVALID),
    ("gsr_mcmc_noise", lambda: _noise_args(n=-1), _INVALID),
    *[("gsr_mcmc_noise", (lambda k=k: _noise_args(**{k: None})), _INVALID) for k in ("xyz", "opacity_logit", "log_scale", "rotation", "noise")],
    *[("gsr_mcmc_noise", (lambda k=k: _noise_args(**{k: _AT + 8})), _INVALID) for k in ("xyz", "log_scale", "rotation", "noise")],
    ("gsr_mcmc_noise", lambda: _noise_args(opacity_logit=_AT + 2), _INVALID),
    ("gsr_mcmc_noise", lambda: _noise_args(n=0, xyz=_AT + 4), _INVALID),                 # (alignment is refused whatever n is)
    ("gsr_mcmc_noise", lambda: _noise_args(n=_BIG), _TOO_LARGE),
    ("gsr_mcmc_plan", lambda: (-1, _AT, 0.0, _AT, _AT, _AT, _AT, None), _INVALID),
    *[("gsr_mcmc_plan", (lambda i=i: tuple(None if j == i else v for j, v in enumerate((5, _AT, 0.0, _AT, _AT, _AT, _AT, None)))), _INVALID)
      for i in (1, 3, 4, 5, 6)],
    ("gsr_mcmc_plan", lambda: (0, None, 0.0, None, None, None, None, None), _INVALID),   # (the counts are written even for n == 0)
    ("gsr_mcmc_plan", lambda: (5, _AT + 2, 0.0, _AT, _AT, _AT, _AT, None), _INVALID),
    ("gsr_mcmc_plan", lambda: (5, _AT, 0.0, _AT + 8, _AT, _AT, _AT, None), _INVALID),   # temp not 16-byte aligned
    ("gsr_mcmc_plan", lambda: (5, _AT, 0.0, _AT, _AT + 2, _AT, _AT, None), _INVALID),
    ("gsr_mcmc_plan", lambda: (5, _AT, 0.0, _AT, _AT, _AT + 1, _AT, None), _INVALID),
    ("gsr_mcmc_plan", lambda: (5, _AT, 0.0, _AT, _AT, _AT, _AT + 2, None), _INVALID),
    ("gsr_mcmc_plan", lambda: (_BIG, _AT, 0.0, _AT, _AT, _AT, _AT, None), _TOO_LARGE),
    ("gsr_mcmc_plan", lambda: (1 << 40, _AT, 0.0, _AT, _AT, _AT, _AT, None), _TOO_LARGE),
    ("gsr_mcmc_relocate", lambda: _relocate_args(struct_size=4), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(n=-1), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(m=-1), _INVALID),
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".param": None})), _INVALID) for k in R.RAW],
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".exp_avg": _AT})), _INVALID) for k in R.RAW],       # one moment alone
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".exp_avg_sq": _AT})), _INVALID) for k in R.RAW],
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".param": _AT + 4})), _INVALID) for k in R.RAW],
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".exp_avg": _AT + 8, k + ".exp_avg_sq": _AT})), _INVALID) for k in R.RAW],
    *[("gsr_mcmc_relocate", (lambda k=k: _relocate_args(**{k + ".exp_avg": _AT, k + ".exp_avg_sq": _AT + 4})), _INVALID) for k in R.RAW],
    ("gsr_mcmc_relocate", lambda: _relocate_args(sampled=None), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(temp=None), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(sampled=_AT + 2), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(dst=_AT + 1), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(temp=_AT + 8), _INVALID),
    ("gsr_mcmc_relocate", lambda: _relocate_args(m=0, temp=_AT + 8), _INVALID),          # (alignment is refused whatever m is)
    *[("gsr_mcmc_relocate", (lambda v=v: _relocate_args(min_opacity=v)), _INVALID) for v in (0.0, 1.0, -0.5, 1.5, float("nan"))],
    ("gsr_mcmc_relocate", lambda: _relocate_args(n=_BIG), _TOO_LARGE),
    ("gsr_mcmc_relocate", lambda: _relocate_args(m=_BIG), _TOO_LARGE),
]


@pytest.mark.parametrize("case", range(len(_REFUSALS)))
def test_mcmc_refusals_come_before_any_hip_call(case):
    name, args, code = _REFUSALS[case]
    L = _capi.lib()
    assert getattr(L, name)(*args()) == code, name
    assert L.gsr_last_error() == code and L.gsr_last_hip_error() == b""


def test_mcmc_temp_bytes():
    L = _capi.lib()
    for fn in (L.gsr_mcmc_plan_temp_bytes, L.gsr_mcmc_relocate_temp_bytes):
        for n in (-1, -(1 << 40), _BIG, 1 << 40):
            assert fn(n) == 0, n
        sizes = [fn(n) for n in (0, 1, 63, 64, 65, 4096, 4097, 1_000_000, 5_834_784, _capi.GSR_MCMC_MAX_ROWS)]
        assert all(s > 0 and s % 16 == 0 for s in sizes) and sizes == sorted(sizes)
    assert L.gsr_mcmc_relocate_temp_bytes(1000) == 16 + 4000                # `rejected` in a 16-byte head, then c[n]
    assert 4 * 1_000_000 <= L.gsr_mcmc_plan_temp_bytes(1_000_000) < 5 * 1_000_000


# ---- the Python refusals: before anything is launched (none of these reaches the library) ----
def test_python_refusals():
    from gsrast_amd.autograd import GaussianParams
    rng = np.random.default_rng(0)
    raw = [rng.normal(size=(6, R.WIDTHS[k]) if k != "opacity_logit" else 6).astype(F) for k in R.RAW]
    params = GaussianParams.from_raw(*raw, device="cpu")
    for call in (lambda: mcmc.inject_noise(params, 1e-3), lambda: mcmc.relocate_dead(params, None),
                 lambda: mcmc.add_new(params, None, cap_max=100)):
        with pytest.raises(ValueError, match="not on a GPU"):
            call()
    with pytest.raises(ValueError, match="one dimension"):
        mcmc.sample_rows(torch.ones(3, 2), torch.zeros(1, dtype=torch.float64))
