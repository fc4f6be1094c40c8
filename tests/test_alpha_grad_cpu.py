"""CPU: the accumulated opacity's gradient (gsr_backward_alpha, include/gsrast_amd_opacity.h). The reference of tests/alpha_grad_ref.py
against central finite differences of sum g_a (1 - finalT) and against the closed form on the opacity; choose_backward with
the new pointer (gsrast_amd/csrc/backward_policy.hpp, compiled with g++ as tests/test_backward_policy.py compiles it); the
new header against its ctypes table, and gsr_backward_args unchanged."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import alpha_grad_ref as A
from helpers import ROOT
from oracle import backward_np as B

from gsrast_amd import _capi

# ---- the reference ------------------------------------------------------------------------------------------------------
STEP_MEAN, STEP_CO = 1e-6, 1e-7
SEED = {1e-3: 2, 1e-4: 5}


def _toy(seed, n=7, w=12, h=10):
    """One tile, a few Gaussians: mixed sizes, three nearly opaque ones so that alpha clamps and pixels terminate."""
    rng = np.random.default_rng(seed)
    means = np.stack([rng.uniform(-1, w + 1, n), rng.uniform(-1, h + 1, n)], 1)
    s = rng.uniform(0.03, 0.4, (n, 2))
    rho = rng.uniform(-0.6, 0.6, n)
    conic = np.stack([s[:, 0], rho * np.sqrt(s[:, 0] * s[:, 1]), s[:, 1]], 1)
    op = rng.uniform(0.05, 0.95, n)
    op[:3] = [1.0, 0.999, 0.98]
    conic[:3] *= 0.25
    co = np.concatenate([conic, op[:, None]], 1)
    plist = rng.permutation(n).astype(np.int64)
    ranges = np.array([[0, n]], np.int64)
    g_a = rng.normal(size=(h, w))
    return means, co, ranges, plist, w, h, g_a


def _undecided_at_the_steps(means, co, ranges, plist, w, h, t_cutoff):
    """True if some decision of the blend loop (see alpha_grad_ref.decisions) comes out differently at one of the points the
    finite differences evaluate: a threshold within the step, where the difference quotient is no derivative."""
    base = A.decisions(means, co, ranges, plist, w, h, t_cutoff)
    for x, step, which in ((means, STEP_MEAN, 0), (co, STEP_CO, 1)):
        for i in range(x.size):
            for sign in (1.0, -1.0):
                y = x.copy()
                y.reshape(-1)[i] += sign * step
                args = (y, co) if which == 0 else (means, y)
                if A.decisions(*args, ranges, plist, w, h, t_cutoff) != base:
                    return True
    return False


@pytest.mark.parametrize("t_cutoff", [1e-3, 1e-4])
def test_alpha_reference_matches_finite_differences(t_cutoff):
    means, co, ranges, plist, w, h, g_a = _toy(SEED[t_cutoff])
    assert not _undecided_at_the_steps(means, co, ranges, plist, w, h, t_cutoff)      # no decision within the step of its threshold
    kinds = {k for row in A.decisions(means, co, ranges, plist, w, h, t_cutoff) for k in row}
    assert kinds >= {0, 2, 3, 4, 5}, kinds       # faint records, composited ones, clamped ones, pixels that end early (this cutoff)
    col = np.zeros((len(means), 3))
    _, ft, nc = B.blend_forward(means, co, col, ranges, plist, w, h, (0, 0, 0), t_cutoff=t_cutoff)
    assert (ft > 0.2).any() and nc.max() >= 3
    got = A.alpha_term(means, co, ranges, plist, nc, ft, w, h, g_a)
    fd_mean = B.finite_difference(lambda x: A.alpha_loss(x, co, ranges, plist, w, h, g_a, t_cutoff), means, STEP_MEAN)
    fd_co = B.finite_difference(lambda x: A.alpha_loss(means, x, ranges, plist, w, h, g_a, t_cutoff), co, STEP_CO)
    for name, an, fd in (("dL_dmean2D", got["dL_dmean2D"], fd_mean), ("dL_dconic", got["dL_dconic"], fd_co[:, :3]),
                         ("dL_dopacity", got["dL_dopacity"], fd_co[:, 3])):
        err, scale = float(np.abs(an - fd).max()), max(1.0, float(np.abs(fd).max()))
        print(name, "max abs err", err, "scale", scale)
        assert np.abs(fd).max() > 0
        assert err <= 2e-5 * scale, name                          # (the bound tests/test_backward_oracle.py holds the colour term to)


@pytest.mark.parametrize("t_cutoff", [1e-3, 1e-4])
def test_alpha_term_alone_has_the_closed_form_on_the_opacity(t_cutoff):
    means, co, ranges, plist, w, h, g_a = _toy(SEED[t_cutoff])
    col = np.zeros((len(means), 3))
    _, ft, nc = B.blend_forward(means, co, col, ranges, plist, w, h, (0, 0, 0), t_cutoff=t_cutoff)
    got = A.alpha_term(means, co, ranges, plist, nc, ft, w, h, g_a)["dL_dopacity"]
    exp = A.opacity_closed_form(means, co, ranges, plist, nc, ft, w, h, g_a)
    assert np.abs(exp).max() > 0
    assert np.abs(got - exp).max() <= 1e-12 * np.abs(exp).max()
    # ... and the superposition leaves the colour call's dL_dcolor alone and adds the term to the rest
    rng = np.random.default_rng(1)
    colors, g_out, bg = rng.uniform(0, 1, (len(means), 3)), rng.normal(size=(3, h, w)), (0.2, 0.5, 0.9)
    full, term = A.superposed(means, co, colors, ranges, plist, nc, ft, w, h, bg, g_out, g_a)
    plain = B.blend_backward(means, co, colors, ranges, plist, nc, ft, w, h, bg, g_out)
    assert np.array_equal(full["dL_dcolor"], plain["dL_dcolor"]) and np.array_equal(term["dL_dopacity"], got)
    assert np.array_equal(full["dL_dopacity"], plain["dL_dopacity"] + got)


def test_seed_form_equals_the_fourth_channel_form():
    """L = sum g_c C_c + T_f (bg . g - g_a) + const: colour gradient g against background bg with the alpha term is the colour
    call with the background's dot product lowered by g_a — one blend_backward with a background chosen so."""
    means, co, ranges, plist, w, h, g_a = _toy(SEED[1e-3])
    rng = np.random.default_rng(3)
    colors = rng.uniform(0, 1, (len(means), 3))
    g_out = np.zeros((3, h, w))
    g_out[1] = 1.0                                               # bg . g = bg_1: lowering bg_1 by g_a needs g_a constant
    ga = np.full((h, w), 0.37)
    _, ft, nc = B.blend_forward(means, co, colors, ranges, plist, w, h, (0, 0, 0))
    full, _ = A.superposed(means, co, colors, ranges, plist, nc, ft, w, h, (0.2, 0.5, 0.9), g_out, ga)
    seeded = B.blend_backward(means, co, colors, ranges, plist, nc, ft, w, h, (0.2, 0.5 - 0.37, 0.9), g_out)
    for k in A.GEOMETRY:
        assert np.abs(full[k] - seeded[k]).max() <= 1e-12 * max(1.0, np.abs(seeded[k]).max()), k


# ---- the training step's reference ---------------------------------------------------------------------------------------------
STEP_CASES = ("gscuda-depth", "inria-3-depth")


def step_weight_alpha():
    import step_frames as S
    return np.random.default_rng(41).normal(size=(S.H, S.W)).astype(np.float32)


@pytest.mark.parametrize("case", STEP_CASES)
def test_linearised_step_reference_is_the_autograd_of_the_quotient_loss(case):
    """What tests/test_gpu_alpha_grad.py compares the training step with — two gradients() calls of tests/step_autograd_ref.py
    fed the quotient's upstream gradients — against torch.autograd of the loss as written, on the CPU oracle's structure of
    the frame (tests/test_step_autograd_cpu.py's): equal but for the float32 rounding of the two upstream maps. And the
    frame's conditions: the dropped pixels stay under the cap of 1 %, the opacity varies over the frame, and the alpha
    term is no rounding matter in any array it reaches."""
    import step_autograd_ref as R
    import step_frames as S
    from test_step_autograd_cpu import frame
    f = frame(case)
    w_a = step_weight_alpha()
    ref = A.step_reference(f["raw"], f["cam"], case, f["structure"], f["w"], w_a, f["wd"])
    assert ref["drop"].sum() <= 0.01 * S.W * S.H
    # (no pixel of these frames lies under the clamp at 1e-3; the opacity varies over the frame, and 1 / opacity^2 with it)
    assert (ref["opacity"] > 1e-3).all() and ref["opacity"].max() > 0.5 and ref["opacity"].max() - ref["opacity"].min() > 0.2
    exact = A.step_quotient_autograd(f["raw"], f["cam"], case, f["structure"], f["w"], w_a, f["wd"], ref["drop"])
    for k, e in exact.items():
        lin = ref["want"][k] + ref["want_alpha"][k]
        scale = float(np.abs(e).max())
        if scale == 0:
            assert not lin.any(), k
            continue
        err = float(np.abs(lin - e).max()) / scale
        share = float(np.abs(ref["want_alpha"][k]).max()) / scale
        print(f"{case}: {k}: linearised against exact {err:.2e}; the alpha term's largest entry is {share:.2f} of the array's")
        assert err <= 1e-6, k                                        # (float32 epsilon 6e-8 on each upstream weight, sums of either sign)
        if k not in ("shs", "cam_pos"):
            assert share > 100 * R.bound(case, k), (k, share)


# ---- choose_backward ----------------------------------------------------------------------------------------------------
# The gradient is the second argument of gsr_backward_alpha (include/gsrast_amd_opacity.h), not a field of gsr_backward_args:
# choose_backward takes it beside the struct. The driver sets the struct's pointers by a bit mask, as tests/test_backward_policy.py's.
POINTERS = [n for n, t in _capi.BackwardArgs._fields_ if isinstance(t, type) and issubclass(t, C.c_void_p) and n != "stream"]

DRIVER = r"""
#include <cstdio>
#include <cstring>
#include "backward_policy.hpp"
using namespace gsr;
int main() {
    static char dummy[16];
    static float g_a[1];
    unsigned flags; unsigned long long mask; int b, e, alpha;
    while (std::scanf("%u %llu %d %d %d", &flags, &mask, &b, &e, &alpha) == 5) {
        gsr_backward_args a;
        std::memset(&a, 0, sizeof(a));
        a.flags = flags; a.num_gaussians = 8; a.width = 17; a.height = 17; a.tile_row_begin = b; a.tile_row_end = e;
@SET_POINTERS@
        BackwardChoice c{};
        const int rc = alpha == 2 ? choose_backward(a, &c) : choose_backward(a, &c, alpha ? g_a : nullptr);
        std::printf("%d %d %d %d %d %d %d %d %d %d\n", rc, c.alpha, c.wide, c.chain, c.depth, c.inria, c.profile, c.depth_inverse,
                    c.d.row_begin, c.d.row_end);
    }
    return 0;
}
""".replace("@SET_POINTERS@", "\n".join(
    f"        if (mask >> {i} & 1) a.{name} = reinterpret_cast<decltype(a.{name})>(dummy);" for i, name in enumerate(POINTERS)))
CHOICE = ["rc", "alpha", "wide", "chain", "depth", "inria", "profile", "depth_inverse", "row_begin", "row_end"]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("alpha_policy")
    (d / "driver.cpp").write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "gsrast_amd", "csrc"),
                           str(d / "driver.cpp"), "-o", str(exe)])
    return str(exe)


def _choose(driver, pointers, flags=0, rows=(0, 0), alpha=0):
    """alpha: 0 = a null gradient, 1 = a gradient, 2 = the call with two arguments (gsr_backward's)."""
    mask = sum(1 << POINTERS.index(p) for p in pointers)
    out = subprocess.check_output([driver], input=f"{flags} {mask} {rows[0]} {rows[1]} {alpha}\n", text=True).split()
    return dict(zip(CHOICE, map(int, out)))


def _legal_sets():
    from test_backward_policy import LEGAL_SETS
    return LEGAL_SETS


@pytest.mark.parametrize("name", ["narrow_sums", "narrow_chain", "wide_all_depth", "inria_shs"])
def test_alpha_follows_the_pointer_and_asks_for_nothing_else(driver, name):
    flags, ptrs, modes = _legal_sets()[name]
    plain, without, given = (_choose(driver, list(ptrs), flags, alpha=k) for k in (2, 0, 1))
    assert plain == without and (without["rc"], without["alpha"]) == (_capi.GSR_OK, 0)
    assert (given["rc"], given["alpha"]) == (_capi.GSR_OK, 1)
    assert {k: v for k, v in given.items() if k != "alpha"} == {k: v for k, v in without.items() if k != "alpha"}
    assert {k: given[k] for k in modes} == modes


def test_every_refusal_is_unchanged_with_the_pointer_set(driver):
    """Each legal set of tests/test_backward_policy.py less one pointer: refused or not exactly as without the gradient —
    dL_dout_color included (the alpha term does not replace the colour gradient)."""
    checked = 0
    for name, (flags, ptrs, _) in _legal_sets().items():
        for gone in ptrs:
            rest = [p for p in ptrs if p != gone]
            rc = _choose(driver, rest, flags, alpha=1)["rc"]
            assert rc == (_capi.GSR_ERR_INVALID_ARG if ptrs[gone] else _capi.GSR_OK), (name, gone)
            assert rc == _choose(driver, rest, flags)["rc"], (name, gone)
            checked += 1
    assert checked > 40
    ptrs = list(_legal_sets()["narrow_sums"][1])
    assert _choose(driver, [p for p in ptrs if p != "dL_dout_color"], alpha=1)["rc"] == _capi.GSR_ERR_INVALID_ARG
    # the band of tile rows (17 x 17 pixels: two rows of tiles) and the flags, with the gradient given
    assert _choose(driver, ptrs, rows=(0, 3), alpha=1)["rc"] == _capi.GSR_ERR_INVALID_ARG
    got = _choose(driver, ptrs, flags=_capi.GSR_FLAG_PROFILE, rows=(1, 2), alpha=1)
    assert (got["rc"], got["alpha"], got["profile"], got["row_begin"], got["row_end"]) == (_capi.GSR_OK, 1, 1, 1, 2)


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _declared_functions():
    import re
    text = open(os.path.join(ROOT, "include", "gsrast_amd_opacity.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol_the_opacity_header_declares():
    L = _capi.lib()
    names = _declared_functions()
    assert names == ["gsr_backward_alpha"]
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd_opacity.h but not exported"
    assert set(_capi.OPACITY_SIGNATURES) == set(names), "ctypes table and header disagree"
    assert not set(_capi.OPACITY_SIGNATURES) & (set(_capi.SIGNATURES) | set(_capi.INIT_SIGNATURES))


def test_the_struct_is_what_it_was_and_the_header_compiles_as_c(tmp_path):
    """gsr_backward_args did not grow (its size is what gsr_backward checks of callers compiled earlier): every field of the
    ctypes mirror at the header's offset, depth_sums_f64 the last; the new header compiles as C beside the first."""
    names = [n for n, _ in _capi.BackwardArgs._fields_]
    body = 'printf("size %zu\\n", sizeof(gsr_backward_args));'
    body += "".join(f'printf("{f} %zu\\n", offsetof(gsr_backward_args, {f}));' for f in names)
    body += "int (*fn)(gsr_backward_args*, const float*) = gsr_backward_alpha; (void)fn;"
    src, obj = tmp_path / "alpha_abi.c", tmp_path / "alpha_abi.o"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_opacity.h"\nint main(void){' + body + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(obj)])
    exe = tmp_path / "alpha_abi"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd_opacity.h"\nint main(void){'
                   + body.split("int (*fn)")[0] + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == C.sizeof(_capi.BackwardArgs)
    for f in names:
        assert int(got[f]) == getattr(_capi.BackwardArgs, f).offset, f
    assert names[-1] == "depth_sums_f64" and "dL_dout_alpha" not in names


def test_the_new_entry_point_keeps_the_error_contract_and_the_struct_size():
    """As tests/test_capi_cpu.py holds every status-returning entry point: a refusal returns its code and leaves it as the last
    error, without a HIP text. A struct of another size is refused with the gradient given as without; none of these calls
    reaches the HIP runtime."""
    L = _capi.lib()
    invalid = _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert L.gsr_backward_alpha(None, None) == invalid
    assert L.gsr_last_error() == invalid and L.gsr_last_hip_error() == b""
    g_a = (C.c_float * 4)()
    a = _capi.BackwardArgs()
    for size in (C.sizeof(_capi.BackwardArgs) - 8, C.sizeof(_capi.BackwardArgs) + 8, 0):
        a.struct_size = size
        assert L.gsr_backward_alpha(C.byref(a), C.addressof(g_a)) == invalid, size
        assert L.gsr_backward(C.byref(a)) == invalid, size
    a.struct_size = C.sizeof(_capi.BackwardArgs)
    assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
    assert L.gsr_backward_alpha(C.byref(a), C.addressof(g_a)) == invalid          # (null pointers: refused by the policy)
    assert L.gsr_last_error() == invalid and L.gsr_last_hip_error() == b""
