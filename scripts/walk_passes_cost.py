"""The passes that walk a drawn frame's sorted lists — gsr_contribution, gsr_absgrad, gsr_features_forward / _backward,
gsr_distortion_forward / _backward — through
this tree's library and through the parent commit's, in one process, one GPU. The parent's library is built from a checkout
of that commit (python -m gsrast_amd.build there) and named with --parent-lib; the passes' signatures are the same in both, so
every entry point binds. Each library gets a rasterizer of its own and draws its own frame. Two parts:
  1. bits. tests/contrib_ref.py's one_tile_scene at list lengths 1, 64, 65 and 257, faint and opaque — one tile: every Gaussian
     receives at most one atomic per slot, so the double sums do not depend on the order anything arrives in — every output of
     the passes: the contribution's four arrays with and without `dominant`; absgrad for a colour gradient and for colour +
     depth + alpha; the feature map, dL_dfeatures without geometry sums, and every output of backward(features=...) (with
     them), at C = 3 and 17; the distortion map, its three moment planes, dL_dvalues without geometry sums and every output of
     backward(distortion=...), at power 1 and 2. On edge_scene() (3 x 2 tiles, partial at both edges) the contribution arrays
     (integer atomics), the feature map, the distortion map and its moments (no atomics). Any difference ends the run with
     exit status 1.
  2. time. The bench frame (1920 x 1080, garden_like), drawn without a tile history so that both sides take the tiles in patch
     order: the passes' own stage_ms (GSR_FLAG_PROFILE) for the contribution with
     and without `dominant`, absgrad with and without depth, and the features forward and backward at C = 3 and 16, the backward
     with and without geometry sums, and the distortion forward and backward at power 2 and 1, the backward with and without
     geometry sums: REPS rounds of parent (a), this tree (a), parent (b), this tree (b). The rule: this tree's
     median (the mean of its two series' medians) may exceed the parent's by no more than the parent's own inter-quartile spread
     over its two series (lowest first quartile to highest third quartile).
Usage: python scripts/walk_passes_cost.py --parent-lib PATH [--reps N] [--splats N] [--out FILE] [--only-bits]
(--out: default profiles/walk_passes_cost.txt)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import contrib_ref  # noqa: E402
from gsrast_amd import _capi, camera  # noqa: E402
from gsrast_amd.contrib import WHAT, contribution_args  # noqa: E402
from gsrast_amd.rasterizer import SplatRasterizer  # noqa: E402

W, H = 1920, 1080
DEV = "cuda:0"


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS = _arg("--reps", 30)
SPLATS = _arg("--splats", bench.DEFAULT_SPLATS)
PARENT = _arg("--parent-lib", None, str)


def load_parent(path):
    """The parent commit's library beside this tree's: every entry point gets this tree's signature."""
    P = C.CDLL(os.path.abspath(path))
    for table in (_capi.SIGNATURES, _capi.INIT_SIGNATURES, _capi.OPACITY_SIGNATURES, _capi.MCMC_SIGNATURES, _capi.CONTRIB_SIGNATURES,
                  _capi.ANTIALIAS_SIGNATURES, _capi.FILTER3D_SIGNATURES, _capi.ABSGRAD_SIGNATURES, _capi.FEATURES_SIGNATURES,
                  _capi.DISTORTION_SIGNATURES):
        for name, (res, args) in table.items():
            fn = getattr(P, name)
            fn.restype, fn.argtypes = res, args
    return P


class Side:
    """One library and the rasterizer made, and every call made, under it."""

    def __init__(self, lib, scene, width, height):
        self.lib = lib
        _capi._lib = lib
        self.r = SplatRasterizer(width, height, device=DEV)
        self.r.configure_from_scene(scene)

    def __call__(self, fn):
        _capi._lib = self.lib
        return fn(self.r)


def contribution(r, names, profile=False):
    """{name: tensor} of one gsr_contribution call into zeros (and the call's stage_ms)."""
    dt = {"weight_sum": torch.int64, "weight_max": torch.int32, "pixels": torch.int64, "dominant": torch.int64}
    arrays = {k: torch.zeros((r.num_gaussians,), dtype=dt[k], device=DEV) for k in names}
    a = contribution_args(r, r.last_receipt, "gscuda", {k: t.data_ptr() for k, t in arrays.items()})
    if profile:
        a.flags |= _capi.GSR_FLAG_PROFILE
    _capi.call("gsr_contribution", C.byref(a), device=r.device)
    torch.cuda.synchronize()
    return arrays, float(a.stage_ms)


def same_bits(what, a, b, bad):
    """Compares two tensors (or dicts of them) bit for bit; the differences are appended to `bad`."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
        for k in a:
            same_bits(f"{what} {k}", a[k], b[k], bad)
        return
    x, y = a.detach().cpu().contiguous().numpy(), b.detach().cpu().contiguous().numpy()
    x, y = x.view(np.uint8), y.view(np.uint8)
    if x.shape != y.shape or (x != y).any():
        bad.append(f"{what}: {int((x != y).sum()) if x.shape == y.shape else 'shapes'} bytes differ")


def bits(P, T, out):
    gen = torch.Generator().manual_seed(11)
    bad, compared = [], 0
    scenes = [(f"one tile, {n} records, {'opaque' if o else 'faint'}", contrib_ref.one_tile_scene(n, o), True)
              for n in (1, 64, 65, 257) for o in (False, True)]
    scenes.append(("edge scene, 40 x 24", contrib_ref.edge_scene(), False))
    for name, (scene, cam), one_tile in scenes:
        sides = [Side(lib, scene, cam.width, cam.height) for lib in (P, T)]
        n, h, w = sides[0].r.num_gaussians, cam.height, cam.width
        gc, gd, ga = (torch.randn(s, generator=gen).to(DEV) for s in ((3, h, w), (h, w), (h, w)))
        zeros = torch.zeros((3, h, w), device=DEV)
        feats = {c: (torch.randn((n, c), generator=gen).to(DEV), torch.randn((c, h, w), generator=gen).to(DEV),
                     torch.randn((c,), generator=gen).to(DEV)) for c in (3, 17)}
        V, GV = torch.randn((n,), generator=gen).to(DEV), torch.randn((h, w), generator=gen).to(DEV)
        got = []
        for side in sides:
            def passes(r):
                r.draw(cam, sh_degree=0, plan="sort", tile_history=False)
                res = {"contribution, all four": contribution(r, WHAT)[0], "contribution, without dominant": contribution(r, WHAT[:3])[0]}
                for c, (F, G, bg) in feats.items():
                    res[f"feature map, C = {c}"] = r.render_features(F, background=bg).clone()
                for q in (1, 2):
                    res[f"distortion map, power {q}"] = r.render_distortion(V, power=q).clone()
                    res[f"distortion moments, power {q}"] = r._distortion_moments[2].clone()
                    if one_tile:           # (each power's backward calls behind its own forward: they read the moments it kept)
                        res[f"dL_dvalues without geometry, power {q}"] = r.distortion_backward(V, GV, power=q).clone()
                        res[f"backward(distortion=...), power {q}"] = {k: v.clone() for k, v in r.backward(zeros, distortion=(V, GV, q)).items()}
                if not one_tile:
                    return res
                res["absgrad, colour"] = r.absgrad(gc).clone()
                res["absgrad, colour + depth + alpha"] = r.absgrad(gc, dL_ddepth=gd, depth=True, dL_dalpha=ga).clone()
                for c, (F, G, bg) in feats.items():
                    res[f"dL_dfeatures without geometry, C = {c}"] = r.features_backward(F, G).clone()
                    res[f"backward(features=...), C = {c}"] = {k: v.clone() for k, v in r.backward(zeros, features=(F, G, bg)).items()}
                return res
            got.append(side(passes))
        before = len(bad)
        same_bits(name, got[0], got[1], bad)
        compared += sum(len(v) if isinstance(v, dict) else 1 for v in got[0].values())
        out.append(f"  {name:<40s}{len(got[0])} results: {'equal bit for bit' if len(bad) == before else 'DIFFERENT'}")
        del sides
    out.append(f"  {compared} arrays compared, {len(bad)} differ")
    out.extend("  DIFFERENT: " + b for b in bad)
    return not bad


def stats(v):
    v = np.asarray(v, np.float64)
    return float(np.median(v)), float(np.percentile(v, 25)), float(np.percentile(v, 75))


def times(P, T, out):
    dev = torch.device(DEV)
    sc, near, far, pos, label = bench.make_scene("garden_like", SPLATS, dev)
    cam = camera.default_camera(W, H, near=near, far=far, position=pos)
    sides = {"parent": Side(P, sc, W, H), "this tree": Side(T, sc, W, H)}
    # (no tile history: with one, the back walks take the forward blend's slow-tiles-first order when the draw sorted one, which
    # depends on the tile times of each side's own earlier draws — the two sides could walk the same frame in different orders)
    for side in sides.values():
        side(lambda r: r.draw(cam, tile_history=False))
    r0 = sides["this tree"].r
    n = r0.num_gaussians
    out.append(f"bench frame ({label}), N = {n}, R = {r0.last_num_rendered}, plan {r0.last_plan}; stage_ms, medians (and quartiles) of {REPS} rounds of "
               "parent (a), this tree (a), parent (b), this tree (b)")
    gen = torch.Generator().manual_seed(7)
    gc, gd = torch.randn((3, H, W), generator=gen).to(dev), torch.randn((H, W), generator=gen).to(dev)
    zeros = torch.zeros((3, H, W), device=dev)
    into2 = torch.empty((n, 2), device=dev)

    def absgrad(depth):
        def run(r):
            r.absgrad(gc, dL_ddepth=gd if depth else None, depth=True if depth else None, into=into2, profile=True)
            return r.last_absgrad_ms
        return run
    passes = {"contribution, all four outputs": lambda r: contribution(r, WHAT, True)[1],
              "contribution, without dominant": lambda r: contribution(r, WHAT[:3], True)[1],
              "absgrad, colour": absgrad(False), "absgrad, colour + depth": absgrad(True)}
    for c in (3, 16):
        F, G = torch.randn((n, c), generator=gen).to(dev), torch.randn((c, H, W), generator=gen).to(dev)
        fmap, dF = torch.empty((c, H, W), device=dev), torch.empty((n, c), device=dev)

        def fwd(r, F=F, fmap=fmap):
            r.render_features(F, into=fmap, profile=True)
            return r.last_features_ms

        def bwd(r, F=F, G=G, dF=dF):
            r.features_backward(F, G, into=dF, profile=True)
            return r.last_features_ms

        def joint(r, F=F, G=G):
            r.backward(zeros, features=(F, G), profile=True)
            return r.last_features_ms
        passes.update({f"features forward, C = {c}": fwd, f"features backward without geometry, C = {c}": bwd,
                       f"features backward with geometry, C = {c}": joint})
    V, GV = torch.randn((n,), generator=gen).to(dev), torch.randn((H, W), generator=gen).to(dev)
    dmap, dV = torch.empty((H, W), device=dev), torch.empty((n,), device=dev)
    for q in (2, 1):
        def dfwd(r, q=q):
            r.render_distortion(V, power=q, into=dmap, profile=True)
            return r.last_distortion_ms

        def dbwd(r, q=q):          # (the moments: those this side's render_distortion of this power kept, the line before this one)
            r.distortion_backward(V, GV, power=q, into=dV, profile=True)
            return r.last_distortion_ms

        def djoint(r, q=q):
            r.backward(zeros, distortion=(V, GV, q), profile=True)
            return r.last_distortion_ms
        passes.update({f"distortion forward, power {q}": dfwd, f"distortion backward without geometry, power {q}": dbwd,
                       f"distortion backward with geometry, power {q}": djoint})
    ok = True
    for name, fn in passes.items():
        series = [("parent", "a"), ("this tree", "a"), ("parent", "b"), ("this tree", "b")]
        for who, _ in series[:2] * 3:                         # warm-up
            sides[who](fn)
        got = {s: [] for s in series}
        for _ in range(REPS):
            for s in series:
                got[s].append(sides[s[0]](fn))
        st = {s: stats(v) for s, v in got.items()}
        parent = 0.5 * (st[("parent", "a")][0] + st[("parent", "b")][0])
        mine = 0.5 * (st[("this tree", "a")][0] + st[("this tree", "b")][0])
        spread = max(st[("parent", "a")][2], st[("parent", "b")][2]) - min(st[("parent", "a")][1], st[("parent", "b")][1])
        within = mine - parent <= spread
        ok = ok and within
        out.append(f"  {name}")
        for s in series:
            out.append(f"    {s[0] + ' (' + s[1] + ')':<16s}{st[s][0]:8.4f} ms ({st[s][1]:.4f} .. {st[s][2]:.4f})")
        out.append(f"    this tree {mine:.4f} ms against the parent {parent:.4f} ms: {1e3 * (mine - parent):+.1f} us; the parent's own spread "
                   f"{1e3 * spread:.1f} us: {'within' if within else 'EXCEEDS'}")
    return ok


def main():
    assert PARENT, "--parent-lib PATH: the parent commit's libgsrast_amd.so"
    T = _capi.lib()
    P = load_parent(PARENT)
    out = [f"the list-walk passes through this tree's library and the parent commit's, {torch.cuda.get_device_name(0)}", "1. bits"]
    ok = bits(P, T, out)
    if "--only-bits" not in sys.argv:
        out.append("2. time")
        ok = times(P, T, out) and ok
    _capi._lib = T
    print("\n".join(out), flush=True)
    path = _arg("--out", os.path.join(ROOT, "profiles", "walk_passes_cost.txt"), str)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
