"""CPU: the reference of adaptive density control (tests/densify_ref.py) against hand-written cases and, in float64, against a
literal torch transcription of the upstream trainer's densify_and_prune; every refusal of gsr_densify_accumulate / _plan /
_apply (before any HIP call); the ctypes mirrors against the header; and, for the seeded scenes tests/test_gpu_densify.py
runs, that the reference itself meets every class — a GPU test over a scene without split parents would test nothing."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import densify_ref as R
from helpers import ROOT

from gsrast_amd import _capi
from gsrast_amd import densify as D

F = np.float32
# thresholds of the hand-written cases: (max_grad, log_dense, logit_min_opacity, log_world, log_shrink), max_screen 10
HAND = tuple(F(v) for v in (1.0, 0.0, -1.0, 2.0, 0.5))


def _rows(rows, dtype=F):
    """rows: (opacity_logit, largest log-scale, grad_accum, denom, max_radii) each -> the arguments of R.densify; the
    other two log-scales are smaller, the rotation is the identity, std = 1, xyz = (i, 0, 0)."""
    n = len(rows)
    raw = {"xyz": np.zeros((n, 3), dtype), "opacity_logit": np.array([r[0] for r in rows], dtype),
           "log_scale": np.stack([np.array([r[1] - 1.0, r[1], r[1] - 2.0], dtype) for r in rows]),
           "rotation": np.tile(np.array([1, 0, 0, 0], dtype), (n, 1)), "shs": np.arange(n * 48, dtype=dtype).reshape(n, 48)}
    raw["xyz"][:, 0] = np.arange(n)
    moments = {k: (np.full_like(raw[k], 0.25), np.full_like(raw[k], 0.5)) for k in R.RAW}
    stats = (np.array([r[2] for r in rows], dtype), np.array([r[3] for r in rows], np.int32), np.array([r[4] for r in rows], np.int32))
    noise = (np.arange(n * 6, dtype=dtype).reshape(n, 2, 3) + 1) / 8
    return raw, moments, stats, noise, np.ones((n, 3), dtype), raw["rotation"].copy()


def _run(rows, max_screen=10, scalars=HAND):
    raw, moments, stats, noise, stds, quats = _rows(rows)
    return R.densify(raw, moments, *stats, scalars, max_screen, noise, stds, quats), raw, noise


SIX = [(0.0, 0.0, 2.0, 2, 3),          # 0: g == max_grad (hot) and m == log_dense (not big): a clone, and kept
       (0.0, 1.0, 3.0, 2, 3),          # 1: hot and big: split, both children live
       (0.0, -1.0, 5.0, 0, 11),        # 2: never seen (denom == 0: g = 0), but seen larger than max_screen: goes unless the test is off
       (0.0, -1.0, np.nan, 1, 3),      # 3: a NaN gradient counts as 0: kept
       (0.0, 2.25, 4.0, 2, 3),         # 4: hot, big, larger than log_world: doomed — but its children (2.25 - 0.5 <= 2) are not
       (-2.0, -1.0, 4.0, 2, 3)]        # 5: hot and small, but transparent: neither it nor its clone


def test_six_rows_one_per_class_and_tie():
    out, raw, noise = _run(SIX)
    assert out["counts"] == (2, 1, 2, 7)
    assert out["src_of"].tolist() == [0, 3, 0, 1, 4, 1, 4]
    assert out["kept"].tolist() == [True, False, False, True, False, False] and out["clone"].tolist() == [True] + [False] * 5
    assert out["split"].tolist() == [False, True, False, False, True, False] and not out["child_doomed"].any()
    assert out["doomed"].tolist() == [False, False, True, False, True, True]
    # kept rows and the clone: the parameter's bits; moments kept / zero
    src = out["src_of"]
    for k in ("opacity_logit", "rotation", "shs"):
        assert np.array_equal(out["raw"][k], raw[k][src])
    m, v = out["moments"]["shs"]
    assert (m[:2] == 0.25).all() and (v[:2] == 0.5).all() and (m[2:] == 0).all() and (v[2:] == 0).all()
    assert np.array_equal(out["raw"]["xyz"][:3], raw["xyz"][src[:3]]) and np.array_equal(out["raw"]["log_scale"][:3], raw["log_scale"][src[:3]])
    # children: identity rotation and unit deviations: xyz + noise[j][k]; log-scales less log_shrink
    for at, (j, k) in zip(range(3, 7), ((0, 0), (1, 0), (0, 1), (1, 1))):
        assert np.array_equal(out["raw"]["xyz"][at], raw["xyz"][src[at]] + noise[j, k])
        assert np.array_equal(out["raw"]["log_scale"][at], raw["log_scale"][src[at]] - F(0.5))
    # the screen tests off: row 2 stays, row 4 is no longer doomed (and is split all the same)
    off, _, _ = _run(SIX, max_screen=0)
    assert off["counts"] == (3, 1, 2, 8) and off["src_of"].tolist() == [0, 2, 3, 0, 1, 4, 1, 4]
    assert off["doomed"].tolist() == [False] * 5 + [True]


@pytest.mark.parametrize("row,counts,src_of", [
    ((0.0, -1.0, 1.0, 2, 3), (1, 0, 0, 1), [0]),                # not hot: kept
    ((-1.5, -1.0, 1.0, 2, 3), (0, 0, 0, 0), []),                # transparent: nothing is left
    ((-1.0, -1.0, 1.0, 2, 3), (1, 0, 0, 1), [0]),               # opacity_logit == logit_min_opacity: not below it
    ((0.0, -1.0, 2.0, 2, 3), (1, 1, 0, 2), [0, 0]),             # hot and small: itself and a clone
    ((0.0, 1.0, 2.0, 2, 3), (0, 0, 1, 2), [0, 0]),              # hot and big: two children
    ((0.0, 2.75, 2.0, 2, 3), (0, 0, 0, 0), []),                 # ... whose children are too large for the world too
    ((0.0, 2.5, 2.0, 2, 3), (0, 0, 1, 2), [0, 0]),              # ... whose children are exactly log_world: not above it
    ((0.0, 1.0, 2.0, 2, 11), (0, 0, 0, 0), []),                 # split, but seen too large: the children inherit the radius
    ((0.0, 1.0, 2.0, 2, 10), (0, 0, 1, 2), [0, 0]),             # max_radii == max_screen: not above it
    ((0.0, 1.0, 1.9999999, 2, 3), (1, 0, 0, 1), [0]),           # g just below max_grad
])
def test_one_row(row, counts, src_of):
    out, _, _ = _run([row])
    assert out["counts"] == counts and out["src_of"].tolist() == src_of


def test_accumulate_reference_by_hand():
    grad = np.array([[3.0, 4.0], [np.nan, np.nan], [1.0, 0.0], [0.0, 0.0]], F)
    radii = np.array([5, 0, 2, -1], np.int32)
    acc, den, big = R.accumulate(grad, radii, 2.0, 0.5, np.array([1, 2, 3, 4], F), np.array([1, 1, 1, 1], np.int32), np.array([9, 9, 1, 9], np.int32))
    assert acc.tolist() == [1.0 + np.sqrt(F(36.0 + 4.0)).astype(F), 2.0, 5.0, 4.0]
    assert den.tolist() == [2, 1, 2, 1] and big.tolist() == [9, 9, 2, 9]


# ---- float64: a literal transcription of the upstream trainer ---------------------------------------------------------------
def _upstream_build_rotation(r):
    q = r / torch.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1] + r[:, 2] * r[:, 2] + r[:, 3] * r[:, 3])[:, None]
    R_ = torch.zeros((q.size(0), 3, 3), dtype=r.dtype)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R_[:, 0, 0] = 1 - 2 * (y * y + z * z)
    R_[:, 0, 1] = 2 * (x * y - r * z)
    R_[:, 0, 2] = 2 * (x * z + r * y)
    R_[:, 1, 0] = 2 * (x * y + r * z)
    R_[:, 1, 1] = 1 - 2 * (x * x + z * z)
    R_[:, 1, 2] = 2 * (y * z - r * x)
    R_[:, 2, 0] = 2 * (x * z - r * y)
    R_[:, 2, 1] = 2 * (y * z + r * x)
    R_[:, 2, 2] = 1 - 2 * (x * x + y * y)
    return R_


def _upstream(t, moments, grad_accum, denom, max_radii, max_grad, min_opacity, extent, max_screen_size, percent_dense, noise_of):
    """densify_and_prune of the upstream trainer over float64 tensors t = {name: [n, w]} (with the radii carried along, as its
    later versions do). noise_of(selected mask) -> [2 S, 3] standard normal samples, child 0 of every parent then child 1."""
    ids = torch.arange(t["xyz"].shape[0])

    def postfix(new, new_ids, radii, new_radii):
        for k in t:
            t[k] = torch.cat((t[k], new[k]), dim=0)
            moments[k] = tuple(torch.cat((a, torch.zeros_like(new[k])), dim=0) for a in moments[k])
        return torch.cat((ids, new_ids)), torch.cat((radii, new_radii))

    def prune_points(mask, radii):
        valid = ~mask
        for k in t:
            t[k] = t[k][valid]
            moments[k] = tuple(a[valid] for a in moments[k])
        return ids[valid], radii[valid]

    grads = grad_accum / denom
    grads[grads.isnan()] = 0.0
    radii = max_radii.clone()
    scaling = lambda: torch.exp(t["log_scale"])
    # densify_and_clone
    selected = torch.where(grads >= max_grad, True, False)
    selected = torch.logical_and(selected, torch.max(scaling(), dim=1).values <= percent_dense * extent)
    ids, radii = postfix({k: t[k][selected] for k in t}, ids[selected], radii, radii[selected])
    # densify_and_split
    padded = torch.zeros(t["xyz"].shape[0], dtype=grads.dtype)
    padded[:grads.shape[0]] = grads
    selected = torch.where(padded >= max_grad, True, False)
    selected = torch.logical_and(selected, torch.max(scaling(), dim=1).values > percent_dense * extent)
    stds = scaling()[selected].repeat(2, 1)
    samples = stds * noise_of(selected)                                    # torch.normal(mean=0, std=stds)
    rots = _upstream_build_rotation(t["rotation"][selected]).repeat(2, 1, 1)
    new = {k: t[k][selected].repeat(2, 1) for k in t}
    new["xyz"] = torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + t["xyz"][selected].repeat(2, 1)
    new["log_scale"] = torch.log(scaling()[selected].repeat(2, 1) / (0.8 * 2))
    ids, radii = postfix(new, ids[selected].repeat(2), radii, radii[selected].repeat(2))
    ids, radii = prune_points(torch.cat((selected, torch.zeros(2 * int(selected.sum()), dtype=torch.bool))), radii)
    # prune
    prune_mask = (torch.sigmoid(t["opacity_logit"]) < min_opacity).squeeze()
    if max_screen_size:
        big_points_vs = radii > max_screen_size
        big_points_ws = scaling().max(dim=1).values > 0.1 * extent
        prune_mask = torch.logical_or(torch.logical_or(prune_mask, big_points_vs), big_points_ws)
    ids, radii = prune_points(prune_mask, radii)
    return ids


@pytest.mark.parametrize("max_screen", [0, 30])
def test_float64_reference_is_the_upstream_procedure(max_screen):
    case = R.seeded_case(600, 77, with_screen=bool(max_screen))
    f64 = lambda a: a.astype(np.float64)
    raw = {k: f64(v) for k, v in case["raw"].items()}
    moments = {k: tuple(f64(a) for a in v) for k, v in case["moments"].items()}
    extent, max_grad, min_opacity, percent_dense = case["extent"], 2e-4, 0.005, 0.01
    scalars = R.plan_scalars(max_grad, min_opacity, extent, percent_dense, dtype=np.float64)
    stds = np.exp(raw["log_scale"])
    quats = raw["rotation"] / np.sqrt((raw["rotation"] ** 2).sum(axis=1))[:, None]
    noise = f64(case["noise"])
    out = R.densify(raw, moments, f64(case["grad_accum"]), case["denom"], case["max_radii"], scalars, max_screen, noise, stds, quats)
    assert min(out["counts"][:3]) > 0 and out["counts"][3] != 600

    def noise_of(selected):
        """The reference's noise laid out for every split parent: rank j among those whose children survive."""
        parents = np.nonzero(selected.numpy())[0]
        assert (parents < 600).all() and np.array_equal(parents, np.nonzero(out["split"])[0])
        z = np.zeros((parents.size, 2, 3))
        live = ~out["child_doomed"][parents]
        z[live] = noise[:int(live.sum())]
        return torch.from_numpy(np.concatenate([z[:, 0], z[:, 1]]))

    t = {k: torch.from_numpy(raw[k].reshape(600, -1).copy()) for k in R.RAW}
    tm = {k: tuple(torch.from_numpy(a.reshape(600, -1).copy()) for a in moments[k]) for k in R.RAW}
    ids = _upstream(t, tm, torch.from_numpy(f64(case["grad_accum"])), torch.from_numpy(case["denom"].astype(np.float64)),
                    torch.from_numpy(case["max_radii"]), max_grad, min_opacity, extent, max_screen, percent_dense, noise_of)
    assert np.array_equal(ids.numpy(), out["src_of"])
    for k in R.RAW:
        want = t[k].numpy().reshape(out["raw"][k].shape)
        assert np.allclose(out["raw"][k], want, rtol=1e-12, atol=1e-12), k
        for a, b in zip(out["moments"][k], tm[k]):
            assert np.array_equal(a, b.numpy().reshape(a.shape)), k


# ---- the seeded scenes of the GPU tests are not blind -----------------------------------------------------------------------
PLAN_SIZES = (1, 64, 65, 1365, 1366, 4097, 12289)            # (tests/test_gpu_densify.py runs these)


def reference_of(n, with_screen=True, moments=True):
    """The float32 reference of the seeded scene of n rows, with the numpy stand-ins of the activations (the GPU tests pass the
    device's); -> (case, result)"""
    case = R.seeded_case(n, 4000 + n, with_screen)
    raw = case["raw"]
    stds = np.exp(raw["log_scale"]).astype(F)
    quats = (raw["rotation"] / np.sqrt((raw["rotation"].astype(np.float64) ** 2).sum(axis=1))[:, None]).astype(F)
    out = R.densify(raw, case["moments"] if moments else {}, case["grad_accum"], case["denom"], case["max_radii"], case["scalars"],
                    case["max_screen"], case["noise"], stds, quats)
    return case, out


@pytest.mark.parametrize("n", PLAN_SIZES)
def test_seeded_scenes_meet_every_class(n):
    case, out = reference_of(n)
    if n == 1:                                               # one row is one class: it is split, and its children live
        assert out["counts"] == (0, 0, 1, 2) and out["src_of"].tolist() == [0, 0]
        return
    split, doomed = out["split"], out["doomed"]
    classes = {"kept": out["kept"], "clone": out["clone"], "split parent": split, "doomed source": doomed,
               "doomed child": out["child_doomed"], "parent doomed, children not": split & doomed & ~out["child_doomed"]}
    sizes = {k: int(v.sum()) for k, v in classes.items()}
    print(f"[densify scene] n={n}: {sizes}, counts {out['counts']}")
    assert all(v > 0 for v in sizes.values()), sizes
    assert np.isnan(case["grad_accum"]).any() and (case["denom"] == 0).any()
    # without the screen tests the plan differs
    _, off = reference_of(n, with_screen=False)
    assert off["counts"] != out["counts"]


# ---- the host's scalars -----------------------------------------------------------------------------------------------------
def test_the_hosts_scalars_are_the_references():
    for max_grad, min_opacity, extent, percent_dense in ((2e-4, 0.005, 4.0, 0.01), (1e-3, 0.05, 17.3, 0.02)):
        got = (C.c_float * 5)(*D.plan_scalars(max_grad, min_opacity, extent, percent_dense))
        want = np.array(R.plan_scalars(max_grad, min_opacity, extent, percent_dense), F)
        assert (np.array(got[:], F).view(np.uint32) == want.view(np.uint32)).all()


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
BAD, TOO_LARGE = _capi.GSR_ERR_INVALID_ARG, 5


def _accumulate_args():
    return dict(n=10, dL_dmean2D=0x10000, radii=0x20000, half_width=64.0, half_height=32.0, grad_accum=0x30000, denom=0x40000,
                max_radii=0x50000, stream=None)


def _plan_args():
    return dict(n=10, opacity_logit=0x10000, log_scale=0x20000, grad_accum=0x30000, denom=0x40000, max_radii=0x50000,
                max_grad=2e-4, log_dense=-3.0, logit_min_opacity=-5.0, log_world=-1.0, log_shrink=0.47, max_screen=20,
                temp=0x60000, src_of=0x70000, counts=0x80000, stream=None)


def _apply_args(moments=True):
    """Arguments gsr_densify_apply accepts, with made-up aligned addresses (no test here lets a call reach a launch)."""
    a = _capi.DensifyApplyArgs()
    a.struct_size, a.log_shrink, a.n_src = C.sizeof(_capi.DensifyApplyArgs), 0.47, 10
    a.counts[:] = [6, 3, 2, 13]
    a.src_of, a.noise = 0x10000, 0x20000
    for i, k in enumerate(R.RAW):
        arr = getattr(a, k)
        fields = [f for f, _ in _capi.DensifyArray._fields_ if moments or "exp" not in f]
        for j, f in enumerate(fields):
            setattr(arr, f, 0x100000 * (i + 1) + 0x1000 * (j + 1))
    return a


def test_accumulate_refuses_bad_arguments_before_any_hip_call():
    L = _capi.lib()
    call = lambda kw: L.gsr_densify_accumulate(*kw.values())
    assert call(dict(_accumulate_args(), n=0)) == _capi.GSR_OK         # the arguments of every refusal below are otherwise these
    assert call(dict(_accumulate_args(), n=-1)) == BAD
    for name in ("dL_dmean2D", "radii", "grad_accum", "denom", "max_radii"):
        assert call(dict(_accumulate_args(), **{name: None})) == BAD, name
        for off in (1, 2, 3):
            assert call(dict(_accumulate_args(), **{name: _accumulate_args()[name] + off})) == BAD, (name, off)
    assert call(dict(_accumulate_args(), dL_dmean2D=0x10004)) == BAD   # a vec2 array
    assert call(dict(_accumulate_args(), n=0, dL_dmean2D=0x10008)) == _capi.GSR_OK
    assert call(dict(_accumulate_args(), n=0, radii=None)) == BAD and L.gsr_last_error() == BAD
    assert call(dict(_accumulate_args(), n=1 << 42)) == TOO_LARGE


def test_plan_refuses_bad_arguments_before_any_hip_call():
    L = _capi.lib()
    call = lambda kw: L.gsr_densify_plan(*kw.values())
    limit = (2 ** 31 - 1) // 3
    pointers = ("opacity_logit", "log_scale", "grad_accum", "denom", "max_radii", "temp", "src_of", "counts")
    assert call(dict(_plan_args(), n=-1)) == BAD
    for name in pointers:
        assert call(dict(_plan_args(), **{name: None})) == BAD, name
        for off in (1, 2, 3):
            assert call(dict(_plan_args(), **{name: _plan_args()[name] + off})) == BAD, (name, off)
    for off in (4, 8, 12):
        assert call(dict(_plan_args(), temp=_plan_args()["temp"] + off)) == BAD, off
    assert call(dict(_plan_args(), n=limit + 1)) == TOO_LARGE and L.gsr_last_error() == TOO_LARGE
    assert call(dict(_plan_args(), n=limit + 1, counts=None)) == BAD   # (a refusal of the arguments comes first)
    # the scratch: the three flag arrays and the scan's; none for what the call refuses
    assert L.gsr_densify_plan_temp_bytes(-1) == 0 and L.gsr_densify_plan_temp_bytes(limit + 1) == 0
    assert L.gsr_densify_plan_temp_bytes(0) == L.gsr_scan_temp_bytes(0)
    for n in (1, 1365, 1366, 5_834_784, limit):
        flags = (12 * n + 127) // 128 * 128
        assert L.gsr_densify_plan_temp_bytes(n) == flags + L.gsr_scan_temp_bytes(3 * n), n


def test_apply_refuses_bad_arguments_before_any_hip_call():
    L = _capi.lib()
    call = lambda a: L.gsr_densify_apply(C.byref(a))
    assert L.gsr_densify_apply(None) == BAD
    for moments in (True, False):
        a = _apply_args(moments)
        a.counts[:] = [0, 0, 0, 0]
        assert call(a) == _capi.GSR_OK                                 # the arguments of every refusal below are otherwise these
    for size in (0, C.sizeof(_capi.DensifyApplyArgs) - 8, C.sizeof(_capi.DensifyApplyArgs) + 8):
        a = _apply_args()
        a.struct_size = size
        assert call(a) == BAD, size
    # counts that do not add up, or that the source cannot give
    for counts in ([6, 3, 2, 12], [6, 3, 2, 14], [-1, 3, 2, 6], [6, -1, 2, 9], [6, 3, -1, 7], [9, 3, 2, 16], [6, 9, 2, 19],
                   [11, 0, 0, 11], [0, 11, 0, 11], [0, 0, 11, 22]):
        a = _apply_args()
        a.counts[:] = counts
        assert call(a) == BAD, counts
    a = _apply_args()
    a.n_src = -1
    assert call(a) == BAD
    for field in ("src_of", "noise"):
        a = _apply_args()
        setattr(a, field, None)
        assert call(a) == BAD, field
        for off in (1, 2, 3):
            a = _apply_args()
            setattr(a, field, getattr(a, field) + off)
            assert call(a) == BAD, (field, off)
    a = _apply_args()                                                  # no split: no noise is needed
    a.counts[:] = [0, 0, 0, 0]
    a.noise = None
    assert call(a) == _capi.GSR_OK
    a.src_of = None
    assert call(a) == BAD and L.gsr_last_error() == BAD
    for k in R.RAW:
        for field, _ in _capi.DensifyArray._fields_:
            a = _apply_args()
            setattr(getattr(a, k), field, None)                        # src / dst missing, or one moment pointer of four
            assert call(a) == BAD, (k, field)
            for off in (4, 8, 12, 1):
                a = _apply_args()
                setattr(getattr(a, k), field, getattr(getattr(a, k), field) + off)
                assert call(a) == BAD, (k, field, off)
        a = _apply_args(moments=False)
        getattr(a, k).dst_exp_avg = 0x900000                           # one of four
        assert call(a) == BAD, k


def test_densify_args_have_the_headers_layout(tmp_path):
    """The header compiled as C prints sizes and offsets: the ctypes mirrors agree field for field."""
    probes = {"gsr_densify_array": (_capi.DensifyArray, [f for f, _ in _capi.DensifyArray._fields_]),
              "gsr_densify_apply_args": (_capi.DensifyApplyArgs, [f for f, _ in _capi.DensifyApplyArgs._fields_])}
    lines = []
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f in fields]
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + "".join(lines) + "return 0;}")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).strip().splitlines())
    for cname, (ctype, fields) in probes.items():
        assert int(got[cname]) == C.sizeof(ctype), cname
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(ctype, f).offset, f"{cname}.{f}"


# ---- the Python layer's refusals that need no GPU ---------------------------------------------------------------------------
def test_python_refusals_on_the_cpu():
    from gsrast_amd.autograd import FrameSlot, GaussianParams, RadiiSlot
    case = R.seeded_case(8, 1)
    params = GaussianParams.from_raw(*(case["raw"][k] for k in R.RAW))
    before = [getattr(params, k) for k in R.RAW]
    stats = D.DensityStats(8, "cpu")
    with pytest.raises(ValueError, match="not on a GPU"):
        D.densify_and_prune(params, None, stats, extent=4.0)
    assert all(getattr(params, k) is p for k, p in zip(R.RAW, before))
    assert issubclass(FrameSlot, RadiiSlot) and FrameSlot().radii is None and FrameSlot().dL_dmean2D is None
    with pytest.raises(ValueError, match="holds no frame"):
        stats.update(FrameSlot(), 64, 64)
    with pytest.raises(ValueError, match="holds no frame"):
        stats.update(RadiiSlot(), 64, 64)
    with pytest.raises(ValueError, match="ceiling"):
        D.reset_opacity(params, None, ceiling=1.0)
    # reset_opacity is plain torch: the CPU runs it
    opt = torch.optim.Adam(params.parameters(), lr=1e-3)
    p = params.opacity_logit
    opt.state[p].update(step=torch.tensor(3.0), exp_avg=torch.ones(8), exp_avg_sq=torch.ones(8))
    version, want = p._version, np.minimum(case["raw"]["opacity_logit"], F(np.log(0.01 / 0.99)))
    D.reset_opacity(params, opt)
    assert p._version > version and (p.detach().numpy().view(np.uint32) == want.view(np.uint32)).all() and (want != case["raw"]["opacity_logit"]).any()
    assert not opt.state[p]["exp_avg"].any() and not opt.state[p]["exp_avg_sq"].any() and opt.state[p]["step"] == 3
