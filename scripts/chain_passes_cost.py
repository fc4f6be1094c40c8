"""The per-Gaussian passes that call csrc/gaussian_chain.hpp — gsr_antialias_forward / _backward, gsr_gaussian_normals_forward /
_backward, the chain stage of gsr_backward, gsr_camera_backward — through this tree's library and through the parent commit's, in
one process, one GPU. The parent's library is built from a checkout of that commit (python -m gsrast_amd.build there) and named
with --parent-lib; the signatures are the same in both, so every entry point binds. Each library gets a rasterizer of its own and
draws its own frame. Two parts:
  1. bits. Any difference, or a listed branch no row takes, ends the run with exit status 1.
     a. antialias forward / backward and Gaussian normals forward / backward (no atomics) at N = 1, 255, 256, 257, both profiles:
        the first N rows of tests/antialias_ref.py's needle scene under its camera (tangents smaller than the projection's for
        gscuda, so that clamped rows pass the frustum test) at scale_modifier 1.7 with quaternions that are not normalised, and of
        tests/normals_ref.py's gaussian_case under a mirrored view; radii with zeros, incoming gradients with zero rows; every
        optional output pointer given and absent. The rows per branch are counted on the host by the numpy references' float32
        decisions, and every N but 1 must have a row in each: radii == 0, a zero gradient, culled, clamped at +limx, -limx, +limy,
        -limy with a gradient flowing; each axis shortest, a flipped normal and one that is not.
     b. gsr_backward's chain on a 16 x 16 one-tile frame (tests/contrib_ref.py's one_tile_scene, where every Gaussian receives at
        most one atomic per sum) at list lengths 1, 64, 65 and 257, for gscuda and for inria at sh_degree 0 to 3: every output of
        backward() with wide_sums on and off, with and without with_cov3D, with outputs= subsets that drop dL_dmeans3D or
        dL_dscales / dL_drotations, with a depth gradient plain and inverse, with dL_dalpha, with camera=True. From length 64 up
        two of the listed Gaussians sit outside 1.3 tan of a camera whose tangents are 0.7 of its projection's, one in x and one
        in y (counted on the host; lengths without both fail). The frame of list length 1 has a second tile with a record of its
        own (a frame of one record blends nothing) and no clamped Gaussian.
  2. time. The bench frame (1920 x 1080, garden_like): REPS rounds of parent (a), this tree (a), parent (b), this tree (b) of
     gsr_backward's chain stage (stage_ms[1]) for gscuda and inria SH 3, each with and without dL_dscales / dL_drotations,
     gsr_camera_backward's stage_ms for both, and — device events around the C call, on the frame's arrays — the antialias forward
     (o' and c; o' alone) and backward (every row live; the frame's radii) and the Gaussian normals forward and backward for both
     profiles. The rule is scripts/walk_passes_cost.py's: this tree's median (the mean of its two series' medians) may exceed the
     parent's by no more than the parent's own inter-quartile spread over its two series.
Usage: python scripts/chain_passes_cost.py --parent-lib PATH [--reps N] [--splats N] [--out FILE] [--only-bits]
(--out: default profiles/chain_passes_cost.txt)"""
import ctypes as C
import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import antialias_ref  # noqa: E402
import bench  # noqa: E402
import contrib_ref  # noqa: E402
import helpers  # noqa: E402
import normals_ref  # noqa: E402
from walk_passes_cost import DEV, H, PARENT, REPS, SPLATS, W, Side, _arg, same_bits, stats  # noqa: E402
from gsrast_amd import _capi, antialias, autograd, backward_plan, camera, normals  # noqa: E402

TABLES = (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
          _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES,
          _capi.DISTORTION_SIGNATURES, _capi.NORMALS_SIGNATURES)
SENTINEL = 7.0                     # what an output tensor holds before a call: rows a call leaves alone compare equal too


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point gets this tree's signature."""
    P = C.CDLL(os.path.abspath(path))
    for table in TABLES:
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    return P


def ccall(lib, name, a):
    with torch.cuda.device(DEV):
        _capi.check(getattr(lib, name)(C.byref(a)), name)


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(device=DEV, dtype=dtype)


def new(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device=DEV)


def ptr(t):
    return t.data_ptr() if t is not None else None


# ---- 1a. the passes of one lane per Gaussian ----------------------------------------------------------------------------------
def seeded_rows(n, seed):
    """(radii int32 [n] with a fifth of the rows 0, a mask of a tenth of the rows whose incoming gradient is zero)."""
    rng = np.random.default_rng(seed)
    radii = np.where(rng.uniform(size=n) < 0.2, 0, rng.integers(1, 40, n)).astype(np.int32)
    return radii, rng.uniform(size=n) < 0.1


def antialias_case(lib, sem, n):
    """({name: tensor} of every call of one library, {branch: rows}) for the first n rows of the needle scene."""
    cam = antialias_ref.camera(sem)
    scene = antialias_ref.first_rows(antialias_ref.needle_scene(sem), n)
    q = scene["rotations"] * np.random.default_rng(40 + n).uniform(0.8, 1.25, (n, 1)).astype(np.float32)
    mod, tan, wh = 1.7, (cam.tan_fovx, cam.tan_fovy), (antialias_ref.W, antialias_ref.H)
    dec = antialias_ref.compensation_f32(scene["means3D"], scene["scales"], q, scene["opacities"], cam.view, cam.proj, *tan, *wh,
                                         semantics=sem, scale_modifier=mod)
    radii, zero_g = seeded_rows(n, 50 + n)
    g = np.random.default_rng(60 + n).normal(size=n).astype(np.float32)
    g[zero_g] = 0.0
    live = (radii > 0) & ~zero_g
    count = {"radii == 0": int((radii == 0).sum()), "zero gradient": int(((radii > 0) & zero_g).sum()),
             "culled": int((live & dec["culled"]).sum())}
    for k, label in (("hi_x", "+limx"), ("lo_x", "-limx"), ("hi_y", "+limy"), ("lo_y", "-limy")):
        count[f"clamped at {label}"] = int((live & dec["flows"] & dec[k]).sum())
    m, s, qd, o = dev(scene["means3D"]), dev(scene["scales"]), dev(q), dev(scene["opacities"])
    view, proj = dev(cam.view), dev(cam.proj)
    gd, rd = dev(g), dev(radii, torch.int32)

    def fill(a):
        antialias._fill(a, n, m, s, qd, o, view, None if sem == "inria" else proj, tan, *wh, sem, mod, torch.device(DEV))
        return a
    res = {}
    for name, with_o, with_c in (("o' and c", True, True), ("o' alone", True, False), ("c alone", False, True)):
        a = fill(_capi.AntialiasArgs())
        o_out, c_out = (new(n) if with_o else None), (new(n) if with_c else None)
        a.opacities_out, a.compensation = ptr(o_out), ptr(c_out)
        ccall(lib, "gsr_antialias_forward", a)
        res["forward, " + name] = {k: t for k, t in (("o_out", o_out), ("c", c_out)) if t is not None}
    names = ("dL_dopacities", "dL_dmeans3D", "dL_dscales", "dL_drotations")
    subsets = [names] + [tuple(k for k in names if k != drop) for drop in names] + [names[:1]]
    for sub, with_radii in [(sub, True) for sub in subsets] + [(names, False)]:
        a = fill(_capi.AntialiasBackwardArgs())
        outs = {k: (new(n) if k == "dL_dopacities" else new(n, 4)) for k in sub}
        a.dL_dopacities_out, a.radii = gd.data_ptr(), (rd.data_ptr() if with_radii else None)
        for k in names:
            setattr(a, k, ptr(outs.get(k)))
        ccall(lib, "gsr_antialias_backward", a)
        res[f"backward, {' '.join(sub)}, {'with' if with_radii else 'without'} radii"] = outs
    torch.cuda.synchronize()
    return res, count


def normals_case(lib, sem, n):
    means, scales, q = normals_ref.gaussian_case(n, seed=3)
    view = normals_ref.random_view(3, mirrored=True)
    _, dec = normals_ref.gaussian_normals_f32(means, scales, q, view, sem)
    radii, zero_g = seeded_rows(n, 70 + n)
    g = normals_ref.seed_gradient((n, 3), seed=8).copy()
    g[zero_g] = 0.0
    live = (radii > 0) & ~zero_g & dec["valid"]
    count = {"radii == 0": int((radii == 0).sum()), "zero gradient": int(((radii > 0) & zero_g).sum())}
    for axis in range(3):
        count[f"axis {axis} shortest"] = int((live & (dec["axis"] == axis)).sum())
    count["flipped"], count["not flipped"] = int((live & dec["flipped"]).sum()), int((live & ~dec["flipped"]).sum())
    m, s, qd, vd, gd, rd = dev(means), dev(scales), dev(q), dev(view), dev(g), dev(radii, torch.int32)
    flags = normals._flags(sem)
    res = {}
    a = _capi.GaussianNormalsArgs()
    normals._fill_gaussians(a, n, m, s, qd, vd, flags, torch.device(DEV))
    out = new(n, 3)
    a.normals = out.data_ptr()
    ccall(lib, "gsr_gaussian_normals_forward", a)
    res["forward"] = out
    for with_radii in (True, False):
        a = _capi.GaussianNormalsBackwardArgs()
        normals._fill_gaussians(a, n, m, s, qd, vd, flags, torch.device(DEV))
        out = new(n, 4)
        a.dL_dnormals, a.radii, a.dL_drotations = gd.data_ptr(), (rd.data_ptr() if with_radii else None), out.data_ptr()
        ccall(lib, "gsr_gaussian_normals_backward", a)
        res[f"backward, {'with' if with_radii else 'without'} radii"] = out
    torch.cuda.synchronize()
    return res, count


def bits_rows(P, T, out):
    bad, compared = [], 0
    for what, case in (("antialias", antialias_case), ("gaussian normals", normals_case)):
        for sem in ("gscuda", "inria"):
            for n in (1, 255, 256, 257):
                (a, count), (b, _) = case(P, sem, n), case(T, sem, n)
                before = len(bad)
                same_bits(f"{what}, {sem}, N = {n}", a, b, bad)
                compared += sum(len(v) if isinstance(v, dict) else 1 for v in a.values())
                missing = [k for k, c in count.items() if c == 0] if n > 1 else []
                bad.extend(f"{what}, {sem}, N = {n}: no row takes the branch '{k}'" for k in missing)
                out.append(f"  {what + ', ' + sem + ', N = ' + str(n):<36s}{len(a)} calls: {'equal bit for bit' if len(bad) == before else 'DIFFERENT OR A BRANCH MISSING'}"
                           f"; rows{' (one row: exempt from the branch count)' if n == 1 else ''}: {', '.join(f'{k} {c}' for k, c in count.items())}")
    out.append(f"  {compared} arrays compared, {len(bad)} findings")
    out.extend("  FINDING: " + b for b in bad)
    return not bad


# ---- 1b. gsr_backward's chain on one tile --------------------------------------------------------------------------------------
TAN_SHARE = 0.7                    # the call's tangents over the projection's: a frame cropped out of a wider projection


def chain_scene(length):
    """(scene, camera, records expected): one_tile_scene with two of its records centred outside 1.3 tan of the camera's tangents,
    one in x and one in y, from length 64 up; every SH coefficient seeded."""
    if length == 1:
        scene, cam = contrib_ref.one_tile_scene(1, False)
        scene, records = {k: v.copy() for k, v in scene.items()}, 2
    else:
        base, cam = contrib_ref.one_tile_scene(length - 2, False)
        edge = helpers.pixel_splats(cam, [15.7, 8.0], [8.0, 15.7], [0.0, 0.0], [1.5, 1.5], [0.3, 0.3], np.array([[0.2, 0.5, 0.8], [0.7, 0.1, 0.4]]))
        scene, records = {k: np.concatenate([base[k], edge[k]]) for k in base}, length
    n = scene["means3D"].shape[0]
    scene["shs"] = np.random.default_rng(90 + length).normal(0.0, 0.3, (n, 48)).astype(np.float32)
    f = np.float32
    cam = dataclasses.replace(cam, tan_fovx=float(f(TAN_SHARE) * f(cam.tan_fovx)), tan_fovy=float(f(TAN_SHARE) * f(cam.tan_fovy)))
    return scene, cam, records


def clamped_listed(scene, cam, radii):
    """(listed Gaussians clamped in x, in y), from the inputs in float64 (the two rows lie 5 % beyond the limit)."""
    V = np.asarray(cam.view, np.float64).reshape(4, 4).T
    t = scene["means3D"][:, :3].astype(np.float64) @ V[:3, :3].T + V[:3, 3]
    listed = np.asarray(radii) > 0
    return (int((listed & (np.abs(t[:, 0] / t[:, 2]) > 1.3 * cam.tan_fovx)).sum()),
            int((listed & (np.abs(t[:, 1] / t[:, 2]) > 1.3 * cam.tan_fovy)).sum()))


def bits_chain(P, T, out):
    gen = torch.Generator().manual_seed(13)
    bad, compared = [], 0
    full = backward_plan.output_set(True)
    for length in (1, 64, 65, 257):
        scene, cam, records = chain_scene(length)
        h, w = cam.height, cam.width
        gc, gd, ga = (torch.randn(s, generator=gen).to(DEV) for s in ((3, h, w), (h, w), (h, w)))
        variants = {"every output": {}, "wide_sums off": {"wide_sums": False}, "without cov3D": {"with_cov3D": False},
                    "without cov3D, wide_sums off": {"with_cov3D": False, "wide_sums": False},
                    "outputs without dL_dmeans3D": {"outputs": tuple(k for k in full if k != "dL_dmeans3D")},
                    "outputs without dL_dscales / dL_drotations": {"outputs": tuple(k for k in full if k not in ("dL_dscales", "dL_drotations"))},
                    "outputs dL_dmean2D, dL_dcov3D, dL_dshs": {"outputs": ("dL_dmean2D", "dL_dcov3D", "dL_dshs")},
                    "depth gradient": {"dL_ddepth": gd, "depth": True}, "inverse depth gradient": {"dL_ddepth": gd, "depth": "inverse"},
                    "dL_dalpha": {"dL_dalpha": ga}, "camera": {"camera": True},
                    "camera, inverse depth, dL_dalpha, wide_sums off": {"camera": True, "dL_ddepth": gd, "depth": "inverse", "dL_dalpha": ga,
                                                                          "wide_sums": False}}
        for sem, deg in (("gscuda", 3), ("inria", 0), ("inria", 1), ("inria", 2), ("inria", 3)):
            sides = [Side(lib, scene, w, h) for lib in (P, T)]
            got, counts = [], None
            for side in sides:
                def passes(r):
                    r.draw(cam, semantics=sem, sh_degree=deg, plan="sort", tile_history=False)
                    if r.last_num_rendered != records:
                        bad.append(f"list length {length}, {sem}: {records} records expected, the frame has {r.last_num_rendered}")
                    res = {"radii": r.map_geometry_state()["radii"].clone()}
                    for name, kw in variants.items():
                        if deg < 3 and name != "every output":         # (the lower degrees differ in the SH part alone)
                            continue
                        res[name] = {k: v.clone() for k, v in r.backward(gc, semantics=sem, sh_degree=deg, **kw).items()}
                    return res
                got.append(side(passes))
            counts = clamped_listed(scene, cam, got[1]["radii"].cpu().numpy())
            name = f"list length {length}{' (and a record in a second tile)' if length == 1 else ''}, {sem}, sh_degree {deg}"
            before = len(bad)
            same_bits(name, got[0], got[1], bad)
            if length > 1 and min(counts) == 0:
                bad.append(f"{name}: listed Gaussians clamped in x {counts[0]}, in y {counts[1]}")
            compared += sum(len(v) if isinstance(v, dict) else 1 for v in got[0].values())
            out.append(f"  {name}: {len(got[0]) - 1} calls: {'equal bit for bit' if len(bad) == before else 'DIFFERENT OR A BRANCH MISSING'}"
                       f"; listed and clamped in x {counts[0]}, in y {counts[1]}")
            del sides
    out.append(f"  {compared} arrays compared, {len(bad)} findings")
    out.extend("  FINDING: " + b for b in bad)
    return not bad


# ---- 2. time ------------------------------------------------------------------------------------------------------------------
def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def race(name, fns, out):
    """REPS rounds of parent (a), this tree (a), parent (b), this tree (b) of fns[who]() -> ms; the verdict of the rule."""
    series = [("parent", "a"), ("this tree", "a"), ("parent", "b"), ("this tree", "b")]
    for who, _ in series[:2] * 3:                         # warm-up
        fns[who]()
    got = {s: [] for s in series}
    for _ in range(REPS):
        for s in series:
            got[s].append(fns[s[0]]())
    st = {s: stats(v) for s, v in got.items()}
    parent = 0.5 * (st[("parent", "a")][0] + st[("parent", "b")][0])
    mine = 0.5 * (st[("this tree", "a")][0] + st[("this tree", "b")][0])
    spread = max(st[("parent", "a")][2], st[("parent", "b")][2]) - min(st[("parent", "a")][1], st[("parent", "b")][1])
    within = mine - parent <= spread
    out.append(f"  {name}")
    for s in series:
        out.append(f"    {s[0] + ' (' + s[1] + ')':<16s}{st[s][0]:8.4f} ms ({st[s][1]:.4f} .. {st[s][2]:.4f})")
    out.append(f"    this tree {mine:.4f} ms against the parent {parent:.4f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own spread "
               f"{1e3 * spread:.1f} us: {'within' if within else 'EXCEEDS'}")
    return within


def times(P, T, out):
    device = torch.device(DEV)
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, device)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    sides = {"parent": Side(P, sc, W, H), "this tree": Side(T, sc, W, H)}
    libs = {"parent": P, "this tree": T}
    gen = torch.Generator().manual_seed(7)
    gc = torch.randn((3, H, W), generator=gen).to(device)
    full = backward_plan.output_set(True)
    lean = tuple(k for k in full if k not in ("dL_dscales", "dL_drotations"))
    ok = True
    for sem in ("gscuda", "inria"):
        # (no tile history: both sides then take the tiles in patch order, as in walk_passes_cost.py)
        for side in sides.values():
            side(lambda r: r.draw(cam, semantics=sem, sh_degree=3, tile_history=False))
        r0 = sides["this tree"].r
        n = r0.num_gaussians
        out.append(f"bench frame ({label}), {sem}, N = {n}, R = {r0.last_num_rendered}, plan {r0.last_plan}; medians (and quartiles) of {REPS} "
                   "rounds of parent (a), this tree (a), parent (b), this tree (b)")
        for name, outputs in (("every output", None), ("without dL_dscales / dL_drotations", lean)):
            def chain(r, outputs=outputs):
                r.backward(gc, semantics=sem, sh_degree=3, outputs=outputs, profile=True)
                return r.last_backward_ms[1]
            ok = race(f"gsr_backward's chain stage, {sem}, {name}", {who: (lambda s=s: s(chain)) for who, s in sides.items()}, out) and ok
        grads = {who: s(lambda r: r.backward(gc, semantics=sem, sh_degree=3)) for who, s in sides.items()}

        def cam_pass(who):
            def run(r):
                r.camera_backward(grads[who], semantics=sem, sh_degree=3, profile=True, sync=True)
                return r.last_camera_ms
            return lambda: sides[who](run)
        ok = race(f"gsr_camera_backward, {sem}", {who: cam_pass(who) for who in sides}, out) and ok

        # the one-lane-per-Gaussian passes on the frame's arrays: device events around the C call
        m, s, q, o = r0.means3D, r0.scales, r0.rotations, r0.opacities
        view, proj, _, tan_x, tan_y = autograd._camera_tensors(cam, device)
        radii = sides["this tree"](lambda r: r.map_geometry_state()["radii"].clone())
        g1, g3 = torch.randn((n,), generator=gen).to(device).abs_().add_(0.1), torch.randn((n, 3), generator=gen).to(device)
        o_out, c_out, d_o, d_m, d_s, d_q, nrm = new(n), new(n), new(n), new(n, 4), new(n, 4), new(n, 4), new(n, 3)

        def aa(cls):
            a = cls()
            antialias._fill(a, n, m, s, q, o, view, None if sem == "inria" else proj, (tan_x, tan_y), W, H, sem, 1.0, device)
            return a
        f_both, f_one, b_all, b_radii = aa(_capi.AntialiasArgs), aa(_capi.AntialiasArgs), aa(_capi.AntialiasBackwardArgs), aa(_capi.AntialiasBackwardArgs)
        f_both.opacities_out, f_both.compensation, f_one.opacities_out = o_out.data_ptr(), c_out.data_ptr(), o_out.data_ptr()
        for b in (b_all, b_radii):
            b.dL_dopacities_out = g1.data_ptr()
            b.dL_dopacities, b.dL_dmeans3D, b.dL_dscales, b.dL_drotations = d_o.data_ptr(), d_m.data_ptr(), d_s.data_ptr(), d_q.data_ptr()
        b_radii.radii = radii.data_ptr()
        nf, nb = _capi.GaussianNormalsArgs(), _capi.GaussianNormalsBackwardArgs()
        for a in (nf, nb):
            normals._fill_gaussians(a, n, m, s, q, view, normals._flags(sem), device)
        nf.normals = nrm.data_ptr()
        nb.dL_dnormals, nb.radii, nb.dL_drotations = g3.data_ptr(), radii.data_ptr(), d_q.data_ptr()
        for name, entry, a in ((f"gsr_antialias_forward, {sem}, o' and c", "gsr_antialias_forward", f_both),
                               (f"gsr_antialias_forward, {sem}, o' alone", "gsr_antialias_forward", f_one),
                               (f"gsr_antialias_backward, {sem}, every row live", "gsr_antialias_backward", b_all),
                               (f"gsr_antialias_backward, {sem}, the frame's radii", "gsr_antialias_backward", b_radii),
                               (f"gsr_gaussian_normals_forward, {sem}", "gsr_gaussian_normals_forward", nf),
                               (f"gsr_gaussian_normals_backward, {sem}, the frame's radii", "gsr_gaussian_normals_backward", nb)):
            ok = race(name, {who: (lambda lib=lib, entry=entry, a=a: timed(lambda: ccall(lib, entry, a))) for who, lib in libs.items()}, out) and ok
    return ok


def main():
    assert PARENT, "--parent-lib PATH: the parent commit's libgsrast_amd.so"
    T = _capi.lib()
    P = load_parent(PARENT)
    out = [f"the per-Gaussian chain passes through this tree's library and the parent commit's, {torch.cuda.get_device_name(0)}",
           "1a. bits: antialias and Gaussian normals"]
    ok = bits_rows(P, T, out)
    out.append("1b. bits: gsr_backward's chain and gsr_camera_backward on one tile")
    ok = bits_chain(P, T, out) and ok
    if "--only-bits" not in sys.argv:
        out.append("2. time")
        ok = times(P, T, out) and ok
    _capi._lib = T
    print("\n".join(out), flush=True)
    path = _arg("--out", os.path.join(ROOT, "profiles", "chain_passes_cost.txt"), str)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
