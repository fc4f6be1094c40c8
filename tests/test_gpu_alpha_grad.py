"""GPU: the gradient of the accumulated opacity, gsr_backward_alpha (include/gsrast_amd_opacity.h; backward(dL_dalpha=...), rasterize / render
with opacity_grad=True). The reference is tests/alpha_grad_ref.py's superposition of two float64 blend backwards
(oracle/backward_np.py, unchanged): the colour one, and one of colours (1, 0, 0) against (g_a, 0, 0) over a zero background.
The frame is tests/test_gpu_depth_backward.py's — 100 x 70 (partial edge tiles), 1200 Gaussians, background (0.2, 0.5, 0.9),
so that the sign of bg . g - g_a shows —, then the frames of several blocks (tests/test_gpu_backward_blocks.py), the scenes at
the blend's decision boundaries (tests/test_gpu_backward_edges.py), the camera pass (tests/camera_grad_ref.py) and the
training step (tests/step_autograd_ref.py), each with the bound its own file holds."""
import numpy as np
import pytest

import alpha_grad_ref as A

pytestmark = pytest.mark.gpu

RTOL = 2e-4       # as tests/test_gpu_depth_backward.py and tests/test_gpu_backward.py: float32 sums in some order against float64
BG = (0.2, 0.5, 0.9)
_cache = {}


def _close(got, exp, what, rtol=RTOL):
    scale = max(1e-6, float(np.abs(exp).max()))
    err = float(np.abs(np.asarray(got, np.float64) - exp).max())
    print(f"[alpha] {what}: max abs err {err:.3e} at scale {scale:.3e} ({err / scale:.2e})")
    assert err <= rtol * scale, f"{what}: max abs err {err} at scale {scale}"


def _numpy(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _gradients(w, h, seed=11):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(3, h, w)).astype(np.float32), rng.normal(size=(h, w)).astype(np.float32),
            rng.normal(size=(h, w)).astype(np.float32))


def _frame(semantics):
    """The frame, its forward state under `semantics` (sorted lists) and the float64 references, computed once and left
    unchanged: colour pass, alpha term, and (on request) the depth pass of a mode."""
    if semantics in _cache:
        return _cache[semantics]
    import torch
    from oracle import backward_np as B
    from test_gpu_depth_backward import _clamped_ptr, _setup
    r, scene, cam, bg = _setup()
    assert bg == BG
    w, h = cam.width, cam.height
    inria = semantics == "inria"
    kw = dict(semantics=semantics, sh_degree=0)
    r.draw(cam, plan="sort", tile_history=False, **kw)
    g = _numpy(r.map_geometry_state())
    im = _numpy(r.map_image_state())
    plist = r.map_binning_state()["values"].cpu().numpy().view(np.uint32).astype(np.int64)
    clamped = r.geom.view(_clamped_ptr(r), 3 * r.num_gaussians, torch.uint8).cpu().numpy().reshape(-1, 3).copy() if inria else None
    ranges = im["ranges"].view(np.uint32).astype(np.int64)
    dL, gd, ga = _gradients(w, h)
    _, ft64, nc64 = B.blend_forward(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, w, h, bg, t_cutoff=1e-4 if inria else 0.001)
    # precondition: at most 2 pixels whose last contributor differs from the float64 forward's
    assert (nc64 != im["nContrib"].view(np.uint32)).sum() <= 2
    assert (nc64 == 0).any() and (ft64 < 0.01).any()          # pixels nothing reaches, and pixels behind an opaque front
    full, term = A.superposed(g["means2D"], g["conicOpacity"], g["rgb"], ranges, plist, nc64, ft64, w, h, bg, dL, ga)
    # blindness guard: the alpha term is no rounding matter in any array compared
    for k in A.GEOMETRY:
        share = float(np.abs(term[k]).max()) / float(np.abs(full[k]).max())
        print(f"[alpha] {semantics}: the alpha term's largest entry is {share:.2f} of {k}'s")
        assert share > 100 * RTOL, (k, share)
    f = dict(r=r, scene=scene, cam=cam, kw=kw, g=g, im=im, plist=plist, ranges=ranges, nc64=nc64, ft64=ft64, clamped=clamped,
             dL=dL, gd=gd, ga=ga, full=full, term=term, depth={}, vis=np.nonzero(g["radii"] > 0)[0], inria=inria,
             t=lambda a: torch.from_numpy(a).cuda())
    _cache[semantics] = f
    return f


def _depth_pass(f, mode):
    if mode not in f["depth"]:
        from oracle import backward_np as B
        from test_depth_cpu import depth_values_f32
        w, h = f["cam"].width, f["cam"].height
        d = depth_values_f32(f["scene"]["means3D"], np.asarray(f["cam"].view, np.float32), mode == "inverse").astype(np.float64)
        g3 = np.zeros((3, h, w))
        g3[0] = f["gd"]
        f["depth"][mode] = B.blend_backward(f["g"]["means2D"], f["g"]["conicOpacity"], np.stack([d, 0 * d, 0 * d], 1), f["ranges"],
                                            f["plist"], f["nc64"], f["ft64"], w, h, (0.0, 0.0, 0.0), g3)
    return f["depth"][mode]


def _draw(f, feed):
    r = f["r"]
    if feed == "sorted":
        r.draw(f["cam"], plan="sort", tile_history=False, **f["kw"])
        assert r.last_lists_written
    else:
        r.draw(f["cam"], plan="blocks", sorted_lists=False, tile_history=False, **f["kw"])
        assert r.last_plan == "blocks" and not r.last_lists_written
    return r


def _check_chain(f, got):
    from helpers import check_backward_chain, check_backward_chain_inria
    cam = f["cam"]
    if f["inria"]:
        check_backward_chain_inria(got, f["g"], f["scene"], cam, cam.width, cam.height, f["vis"], 0, f["clamped"])
    else:
        check_backward_chain(got, f["g"], f["scene"], cam, cam.width, cam.height, f["vis"])


def _check_sums(got, exp, what, extra=None):
    extra = extra or {k: 0.0 for k in A.GEOMETRY}
    _close(got["dL_dmean2D"], exp["dL_dmean2D"] + extra["dL_dmean2D"], f"{what}: dL_dmean2D")
    _close(got["dL_dconic_opacity"][:, :3], exp["dL_dconic"] + extra["dL_dconic"], f"{what}: dL_dconic")
    _close(got["dL_dconic_opacity"][:, 3], exp["dL_dopacity"] + extra["dL_dopacity"], f"{what}: dL_dopacity")
    _close(got["dL_dcolors"], exp["dL_dcolor"], f"{what}: dL_dcolors")


CASES = [(s, f, w) for s in ("gscuda", "inria") for f in ("sorted", "block_lists") for w in (True, False)]


@pytest.mark.parametrize("semantics,feed,wide", CASES)
def test_alpha_backward_matches_the_float64_superposition(semantics, feed, wide):
    f = _frame(semantics)
    r = _draw(f, feed)
    got = _numpy(r.backward(f["t"](f["dL"]), dL_dalpha=f["t"](f["ga"]), wide_sums=wide, **f["kw"]))
    assert "dL_ddepths" not in got
    _check_sums(got, f["full"], f"{semantics}/{feed}/wide={wide}")
    _check_chain(f, got)


@pytest.mark.parametrize("semantics,mode,feed,wide", [("gscuda", True, "sorted", True), ("gscuda", "inverse", "block_lists", False),
                                                      ("inria", "inverse", "sorted", True), ("inria", True, "block_lists", True)])
def test_alpha_and_depth_gradients_together(semantics, mode, feed, wide):
    from test_depth_cpu import depth_mean_term
    f = _frame(semantics)
    exp_d = _depth_pass(f, mode)
    r = _draw(f, feed)
    got = _numpy(r.backward(f["t"](f["dL"]), dL_ddepth=f["t"](f["gd"]), depth=mode, dL_dalpha=f["t"](f["ga"]), wide_sums=wide,
                            **f["kw"]))
    what = f"{semantics}/{mode}/{feed}/wide={wide}, depth and alpha"
    _check_sums(got, f["full"], what, extra=exp_d)
    _close(got["dL_ddepths"], exp_d["dL_dcolor"][:, 0], f"{what}: dL_ddepths")        # (the opacity does not reach d_i)
    term = depth_mean_term(f["scene"]["means3D"][:, :3], np.asarray(f["cam"].view, np.float32), got["dL_ddepths"], mode == "inverse")
    chain = dict(got)
    chain["dL_dmeans3D"] = got["dL_dmeans3D"].copy()
    chain["dL_dmeans3D"][:, :3] -= term
    _check_chain(f, chain)


@pytest.mark.parametrize("feed,wide", [("sorted", True), ("block_lists", False)])
def test_alpha_alone_with_a_zero_colour_gradient(feed, wide):
    f = _frame("gscuda")
    r = _draw(f, feed)
    import torch
    zeros = torch.zeros((3, f["cam"].height, f["cam"].width), device="cuda")
    got = _numpy(r.backward(zeros, dL_dalpha=f["t"](f["ga"]), wide_sums=wide, **f["kw"]))
    what = f"alpha alone, {feed}, wide={wide}"
    _close(got["dL_dmean2D"], f["term"]["dL_dmean2D"], f"{what}: dL_dmean2D")
    _close(got["dL_dconic_opacity"][:, :3], f["term"]["dL_dconic"], f"{what}: dL_dconic")
    _close(got["dL_dconic_opacity"][:, 3], f["term"]["dL_dopacity"], f"{what}: dL_dopacity")
    assert not got["dL_dcolors"].any() and not got["dL_dshs"].any()      # the opacity does not depend on the colours: exact zeros
    culled = f["g"]["radii"] <= 0
    assert culled.sum() > 0
    for k, v in got.items():
        assert not v[culled].any(), (what, k)
    _check_chain(f, got)
    assert np.abs(got["dL_dmeans3D"]).max() > 0 and np.abs(got["dL_dscales"]).max() > 0


@pytest.mark.parametrize("wide", [True, False])
@pytest.mark.parametrize("feed", ["sorted", "block_lists"])
def test_no_alpha_gradient_equals_a_gradient_of_zeros(feed, wide):
    """dL_dalpha=None (the call as it was before the field existed) against a tensor of zeros: run-to-run differences only."""
    import torch
    f = _frame("gscuda")
    r = _draw(f, feed)
    dL = f["t"](f["dL"])
    a = _numpy(r.backward(dL, wide_sums=wide, **f["kw"]))
    b = _numpy(r.backward(dL, dL_dalpha=torch.zeros((f["cam"].height, f["cam"].width), device="cuda"), wide_sums=wide, **f["kw"]))
    assert sorted(a) == sorted(b)
    for k in a:       # (float atomics, or double ones rounded once: the bounds of tests/test_gpu_depth_backward.py)
        _close(b[k], a[k].astype(np.float64), f"None against zeros, {feed}, wide={wide}: {k}", rtol=1e-6 if wide else 1e-5)
    _check_sums(a, {**{k: f["full"][k] - f["term"][k] for k in A.GEOMETRY}, "dL_dcolor": f["full"]["dL_dcolor"]},
                f"no alpha gradient, {feed}, wide={wide}")


def test_alpha_sums_are_reproducible_and_leave_the_double_sums_zero():
    f = _frame("gscuda")
    r = _draw(f, "sorted")
    dL, gd, ga = f["t"](f["dL"]), f["t"](f["gd"]), f["t"](f["ga"])
    runs = [_numpy(r.backward(dL, dL_dalpha=ga, dL_ddepth=gd, depth="inverse", **f["kw"])) for _ in range(3)]
    for run in runs[1:]:
        for k in run:
            assert np.array_equal(run[k].view(np.uint32), runs[0][k].view(np.uint32)), k
    assert bool((r._bw.scratch["sums_f64"] == 0).all()) and bool((r._bw.scratch["depth_sums_f64"] == 0).all())


# ---- frames of several blocks (tests/test_gpu_backward_blocks.py): per-entry sums and direct atomics in one launch -----------
def _block_frame():
    """Scene A13 of tests/test_gpu_backward_blocks.py with that module's own frame (built once per session, shared with its
    tests) and the per-Gaussian reference of colour + alpha."""
    import helpers as Hh
    import test_gpu_backward_blocks as TB
    f = TB._frame("A13")
    if "alpha" not in _cache:
        w, h = f["cam"].width, f["cam"].height
        ga = np.random.default_rng(23).normal(size=(h, w)).astype(np.float32)
        g3 = np.zeros_like(f["dL_host"])
        g3[0] = ga
        n = f["r"].num_gaussians
        ones = np.zeros((n, 3))
        ones[:, 0] = 1.0
        ref_a = Hh.oracle_gradients(f["snap"], g3, TB.BG, f["tiles"], f["targets"], 4096, f32_forward=True, magnitudes=True,
                                    t_cutoff=f["cutoff"], full_lists=True, colors=ones, background=(0.0, 0.0, 0.0),
                                    threads=TB.THREADS)
        ref = Hh.depth_superposition(f["ref"], ref_a)        # (linear in the colours: the sums and their condition scales add)
        assert np.abs(ref_a["exp"]["dL_dopacity"]).max() > 0 and np.array_equal(ref["exp"]["dL_dcolors"], f["ref"]["exp"]["dL_dcolors"])
        import torch
        _cache["alpha"] = (ga, torch.from_numpy(ga).cuda(), ref)
    return (f,) + _cache["alpha"]


@pytest.mark.parametrize("wide", [True, False], ids=["wide sums", "float sums"])
def test_alpha_on_a_frame_of_several_blocks(wide):
    import helpers as Hh
    import test_gpu_backward_blocks as TB
    f, _, ga, ref = _block_frame()
    facts = f["facts"][False]
    Hh.assert_block_ways(facts, TB.WAYS_MIXED, "A13")         # block (0, 0) direct atomics, the other five per-entry sums
    r = TB._draw_block_fed(f, lists=False)
    im = r.map_image_state()
    what = f"A13, block lists, alpha, {'wide' if wide else 'float'} sums"
    Hh.assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), ref, what)
    got = r.backward(f["dL"], dL_dalpha=ga, wide_sums=wide, **f["kw"])
    TB._check(f, got, ref, facts, wide, what)


def test_alpha_of_two_bands_adds_up_to_the_frame():
    """Tile rows 0 .. 3 and 3 .. 9 of A13 (the cut goes through block row 0): the two calls' gradients, added, are the whole
    frame's — held to the whole frame's reference and bound, the float-sum term where a block may have taken per-entry sums."""
    import helpers as Hh
    import test_gpu_backward_blocks as TB
    f, _, ga, ref = _block_frame()
    total = None
    maybe_float = np.zeros(len(f["targets"]), bool)
    for rows in ((0, TB.BAND[0]), TB.BAND):
        facts = Hh.block_feed_facts(f["snap"], rows=rows)
        per_entry = {k for k, b in facts["blocks"].items() if b["way"] != "direct"}
        maybe_float |= np.array([any(k in per_entry for k in facts["membership"].get(int(g), ())) for g in f["targets"]], bool)
        r = TB._draw_block_fed(f, lists=False, rows=rows)
        got = Hh.gradients_of(r.backward(f["dL"], dL_dalpha=ga, tile_rows=rows, wide_sums=True, **f["kw"]), f["targets"])
        assert all(np.abs(v).max() > 0 for v in got.values()), rows
        total = got if total is None else {k: total[k].astype(np.float64) + got[k] for k in got}
    Hh.assert_backward_per_gaussian(total, ref, float_tile_sums=maybe_float, what="A13, two bands added, alpha")


# ---- the blend's decision boundaries (tests/test_gpu_backward_edges.py) ------------------------------------------------------
@pytest.mark.parametrize("name", ["clamp", "termination", "termination, cut-off 1e-4"])
def test_alpha_at_a_saturated_record_and_an_early_terminated_pixel(name):
    import torch
    import helpers as Hh
    import test_gpu_backward_edges as TE
    from gsrast_amd.rasterizer import SplatRasterizer
    build, semantics = TE.SCENES[name]
    scene, cam = build()
    W, H = cam.width, cam.height
    bg = (0.3, 0.1, 0.6)
    cutoff = 1e-4 if semantics == "inria" else 1e-3
    kw = dict(semantics=semantics, sh_degree=0)
    r = SplatRasterizer(W, H, background=bg)
    r.configure_from_scene(scene)
    n = r.num_gaussians
    rng = np.random.default_rng(29)
    dL, ga = rng.normal(size=(3, H, W)).astype(np.float32), rng.normal(size=(H, W)).astype(np.float32)
    assert (ga != 0).all()
    r.draw(cam, plan="sort", tile_history=False, **kw)
    tiles = [(tx, ty) for ty in range((H + 15) // 16) for tx in range((W + 15) // 16)]
    targets = np.arange(n)
    opts = dict(f32_forward=True, magnitudes=True, t_cutoff=cutoff, full_lists=True)
    ref_c = Hh.oracle_gradients(r, dL, bg, tiles, targets, 4096, **opts)
    g3 = np.zeros_like(dL)
    g3[0] = ga
    ones = np.zeros((n, 3))
    ones[:, 0] = 1.0
    ref_a = Hh.oracle_gradients(r, g3, bg, tiles, targets, 4096, colors=ones, background=(0.0, 0.0, 0.0), **opts)
    ref = Hh.depth_superposition(ref_c, ref_a)
    if name == "clamp":
        TE._edge_clamp(ref)                                    # a Gaussian clamped on every pixel it composites; raw crossing 0.99
    else:
        TE._edge_termination(ref, W, H)
        assert (ref["stop_idx"] >= 0).sum() >= 20                                 # pixels ended at the cut-off, g_a != 0 there
    for vname, dkw, wide in (("sorted list", dict(plan="sort"), True), ("sorted list, float sums", dict(plan="sort"), False),
                             ("block lists", dict(plan="blocks", sorted_lists=False), True)):
        r.draw(cam, tile_history=False, **dkw, **kw)
        im = r.map_image_state()
        Hh.assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), ref, f"{name}, {vname}")
        got = r.backward(torch.from_numpy(dL).cuda(), dL_dalpha=torch.from_numpy(ga).cuda(), wide_sums=wide, **kw)
        Hh.assert_backward_per_gaussian(Hh.gradients_of(got, targets), ref, float_tile_sums=not wide, what=f"{name}, {vname}, alpha")


# ---- the camera ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", ["gscuda", "inria"])
def test_camera_gradient_with_the_alpha_term(semantics):
    """backward(dL_dalpha=..., camera=True) against tests/camera_grad_ref.py fed the float64 superposed per-Gaussian gradients
    (the covariance gradient as -K dL/dK K of the float64 conic gradient): within 2e-4 of the largest entry, the bound of
    tests/test_gpu_camera_grad.py's end-to-end test."""
    from camera_grad_ref import ZERO_ENTRIES, camera_grad
    f = _frame(semantics)
    r, cam = _draw(f, "sorted"), f["cam"]
    out = r.backward(f["t"](f["dL"]), dL_dalpha=f["t"](f["ga"]), camera=True, **f["kw"])
    got = np.concatenate([out[k].cpu().numpy() for k in ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")])

    def reference(sums):
        co = f["g"]["conicOpacity"].astype(np.float64)
        d_conic = sums["dL_dconic"]
        K = np.stack([np.stack([co[:, 0], co[:, 1]], 1), np.stack([co[:, 1], co[:, 2]], 1)], 1)
        gK = np.stack([np.stack([d_conic[:, 0], 0.5 * d_conic[:, 1]], 1), np.stack([0.5 * d_conic[:, 1], d_conic[:, 2]], 1)], 1)
        gM = -K @ gK @ K
        return camera_grad(r.means3D, cam.view, cam.proj, cam.cam_pos, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height,
                           f["g"]["radii"], f["g"]["cov3D"], sums["dL_dmean2D"], np.stack([gM[:, 0, 0], gM[:, 0, 1], gM[:, 1, 1]], 1),
                           inria=f["inria"], shs=r.shs if f["inria"] else None, sh_degree=0,
                           dL_dcolors=f["full"]["dL_dcolor"] if f["inria"] else None, clamped=f["clamped"].astype(bool) if f["inria"] else None)[0]
    exp, alone = reference(f["full"]), reference(f["term"])
    scale, err = float(np.abs(exp).max()), float(np.abs(got - exp).max())
    print(f"[alpha] camera, {semantics}: max abs err {err:.3e} at scale {scale:.3e}; the alpha term's largest entry {np.abs(alone).max():.3e}")
    assert np.abs(alone[:16]).max() > 100 * 2e-4 * scale and np.abs(alone[16:32]).max() > 100 * 2e-4 * scale      # blindness guard
    assert scale > 0 and err <= 2e-4 * scale
    assert (got[ZERO_ENTRIES] == 0).all()


# ---- autograd ----------------------------------------------------------------------------------------------------------------
def _opacity_step(case):
    """One training step with loss (w . color).sum() + (w_a . opacity).sum() + (w_d . depth / opacity.clamp_min(1e-3)).sum()
    under opacity_grad=True, on a frame of tests/step_frames.py. Both sides are handed the quotient's upstream gradients
    dL/ddepth and dL/dopacity, computed in float64 from the reference's maps, so that the loss compared is linear in the maps.
    Returns (got, want, want of the alpha term, the dropped pixels, the structure)."""
    import torch
    import step_autograd_ref as R
    import step_frames as S
    from gsrast_amd.autograd import GaussianParams, render
    from gsrast_amd.rasterizer import SplatRasterizer
    from test_gpu_step_autograd import DRAW, _state
    profile, deg, depth, mod, kx, precomp = S.CASES[case]
    assert depth is True and not precomp
    raw, cam = S.raw_scene(profile), S.camera_of(case)
    dev = torch.device("cuda:0")
    leaf = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32).copy()).to(dev).requires_grad_(True)
    view, proj, pos = leaf(cam.view), leaf(cam.proj), leaf(cam.cam_pos)
    rast = SplatRasterizer(S.W, S.H, background=S.BG)
    params = GaussianParams.from_raw(*(raw[k] for k in S.RAW), sh_layout="coefficient_major" if profile == "inria" else "file", device=dev)
    color, dmap, opac = render(params, rast, (view, proj, pos, cam.tan_fovx, cam.tan_fovy), semantics=profile, sh_degree=deg,
                               scale_modifier=mod, depth=depth, opacity_grad=True, **DRAW)
    assert opac.requires_grad and dmap.requires_grad
    tensors = {k: getattr(params, k) for k in S.RAW}
    tensors.update(view=view, proj=proj, cam_pos=pos)
    g, im, plist, clamped = _state(rast)
    structure = S.structure_of(raw, cam, g["radii"], im["ranges"], plist, im["nContrib"], clamped if profile == "inria" else None)
    from test_alpha_grad_cpu import step_weight_alpha
    w, w_d = S.weights()
    ref = A.step_reference(raw, cam, case, structure, w, step_weight_alpha(), w_d)
    want, want_a, drop, up_depth, up_opac = ref["want"], ref["want_alpha"], ref["drop"], ref["up_depth"], ref["up_opacity"]
    keep = ~drop
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    k = t(keep)
    torch.autograd.backward([color, dmap, opac], [t(w) * k, t(up_depth) * k, t(up_opac) * k])
    torch.cuda.synchronize()
    got = {n: x.grad.detach().cpu().numpy().astype(np.float64) for n, x in tensors.items()}
    return got, want, want_a, drop, structure


@pytest.mark.parametrize("case", ["gscuda-depth", "inria-3-depth"])
def test_training_step_with_the_opacity_gradient_matches_the_float64_autograd_reference(case):
    import step_autograd_ref as R
    import step_frames as S
    from camera_grad_ref import ZERO_ENTRIES
    got, want, want_a, drop, structure = _opacity_step(case)
    assert drop.sum() <= 0.01 * S.W * S.H, int(drop.sum())           # the cap of tests/test_gpu_step_autograd.py
    for k, a in got.items():
        ref = (want[k] + want_a[k]).reshape(a.shape)
        scale = float(np.abs(ref).max())
        if scale == 0:                                               # (the reference's profile does not read cam_pos)
            assert (a == 0).all(), (case, k)
            continue
        err, b = float(np.abs(a - ref).max()) / scale, R.bound(case, k)
        share = float(np.abs(want_a[k]).max()) / scale
        print(f"[alpha] step {case}: {k}.grad worst error {err:.3e} of the largest entry = {err / b:.3f} of the bound; the alpha "
              f"term's largest entry is {share:.2f} of it")
        assert np.isfinite(a).all() and err <= b, (case, k, err, b)
        if k not in ("shs", "cam_pos"):                              # (the opacity does not reach the colours)
            assert share > 100 * b, (case, k, share)                 # blindness guard
    culled = ~structure["vis"]
    for k, a in got.items():
        if k not in ("view", "proj", "cam_pos"):
            assert (a[culled] == 0).all(), (case, k)
    cam35 = np.concatenate([got["view"].reshape(-1), got["proj"].reshape(-1), got["cam_pos"].reshape(-1)])
    assert (cam35[ZERO_ENTRIES] == 0).all(), case


def test_quotient_loss_is_the_linear_step_of_its_own_upstream_gradients():
    """The loss as a user writes it, depth / opacity.clamp_min(1e-3), against the step handed that quotient's gradients with
    respect to the two maps (torch's, on detached copies of the same maps): the same bits — sorted lists and double sums are
    reproducible, and the opacity's gradient is nothing but an input of gsr_backward."""
    import torch
    import step_frames as S
    from gsrast_amd.autograd import GaussianParams, render
    from gsrast_amd.rasterizer import SplatRasterizer
    from test_gpu_step_autograd import DRAW
    raw, cam = S.raw_scene("gscuda"), S.camera_of("gscuda-depth")
    dev = torch.device("cuda:0")
    w, w_d = (torch.from_numpy(a).to(dev) for a in S.weights())
    w_a = torch.from_numpy(np.random.default_rng(41).normal(size=(S.H, S.W)).astype(np.float32)).to(dev)
    loss_of = lambda c, d, o: (w * c).sum() + (w_a * o).sum() + (w_d * d / o.clamp_min(1e-3)).sum()
    rast = SplatRasterizer(S.W, S.H, background=S.BG)
    grads = []
    for linear in (False, True):
        params = GaussianParams.from_raw(*(raw[k] for k in S.RAW), device=dev)
        color, dmap, opac = render(params, rast, cam, depth=True, opacity_grad=True, **DRAW)
        if linear:
            maps = [t.detach().clone().requires_grad_(True) for t in (color, dmap, opac)]
            torch.autograd.backward([color, dmap, opac], list(torch.autograd.grad(loss_of(*maps), maps)))
        else:
            loss_of(color, dmap, opac).backward()
        torch.cuda.synchronize()
        grads.append({k: getattr(params, k).grad.cpu().numpy() for k in S.RAW})
    assert bool((opac > 0.5).any()) and float((opac.max() - opac.min()).detach()) > 0.2
    for k in S.RAW:
        assert np.abs(grads[0][k]).max() > 0 or k == "shs"
        assert np.array_equal(grads[0][k].view(np.uint32), grads[1][k].view(np.uint32)), k


# ---- the interface -----------------------------------------------------------------------------------------------------------
def test_default_render_keeps_the_opacity_map_out_of_the_graph():
    import torch
    import step_frames as S
    from gsrast_amd.autograd import GaussianParams, render
    from gsrast_amd.rasterizer import SplatRasterizer
    raw, cam = S.raw_scene("gscuda"), S.camera_of("gscuda")
    params = GaussianParams.from_raw(*(raw[k] for k in S.RAW), device="cuda:0")
    rast = SplatRasterizer(S.W, S.H, background=S.BG)
    color, _, opac = render(params, rast, cam)
    assert color.requires_grad and not opac.requires_grad and opac.grad_fn is None
    with pytest.raises(RuntimeError, match="does not require grad"):
        opac.sum().backward()
    color2, _, opac2 = render(params, rast, cam, opacity_grad=True)
    assert opac2.requires_grad and opac2.data_ptr() != opac.data_ptr()          # a new tensor of the call
    assert torch.equal(opac2.detach(), opac) and torch.equal(color2.detach(), color.detach())
    # a loss on the colour alone under opacity_grad=True is the default call's, bit for bit (no gradient of zeros is run through)
    w = torch.randn((3, S.H, S.W), generator=torch.Generator().manual_seed(3)).cuda()
    grads = []
    for kw in ({}, {"opacity_grad": True}):
        p2 = GaussianParams.from_raw(*(raw[k] for k in S.RAW), device="cuda:0")
        (w * render(p2, rast, cam, plan="sort", tile_history=False, **kw)[0]).sum().backward()
        grads.append({k: getattr(p2, k).grad.cpu().numpy() for k in S.RAW})
    for k in S.RAW:
        assert np.array_equal(grads[0][k].view(np.uint32), grads[1][k].view(np.uint32)), k
    color2, _, opac2 = render(params, rast, cam, opacity_grad=True)
    opac2.sum().backward()                                                      # the opacity alone: no colour gradient at all
    assert params.opacity_logit.grad is not None and float(params.opacity_logit.grad.abs().max()) > 0
    assert float(params.xyz.grad.abs().max()) > 0 and not bool(params.shs.grad.any())
    assert float(params.opacity_logit.grad.min()) >= 0                           # more opaque Gaussians never lower 1 - T


def test_refusals_of_the_alpha_gradient():
    """A wrong shape, dtype or device is refused before anything is launched: the output buffers of the call before are untouched."""
    import torch
    f = _frame("gscuda")
    r = _draw(f, "sorted")
    h, w = f["cam"].height, f["cam"].width
    dL = f["t"](f["dL"])
    held = r.backward(dL, **f["kw"])                                  # (this object's output tensors: the next call overwrites them)
    before = _numpy(held)
    good = torch.zeros((h, w), device="cuda")
    for what, bad in (("transposed", torch.zeros((w, h), device="cuda")), ("three planes", torch.zeros((3, h, w), device="cuda")),
                      ("flat", torch.zeros(h * w, device="cuda")), ("float64", good.double()), ("float16", good.half()),
                      ("on the host", good.cpu()), ("numpy", np.zeros((h, w), np.float32))):
        with pytest.raises(AssertionError):
            r.backward(dL * 2.0, dL_dalpha=bad, **f["kw"])
        torch.cuda.synchronize()
        after = _numpy(held)
        assert all(np.array_equal(after[k].view(np.uint32), before[k].view(np.uint32)) for k in before), what
    # a view that is not contiguous is copied, not refused
    wide = torch.zeros((h, 2 * w), device="cuda")
    wide[:, ::2] = f["t"](f["ga"])
    a = _numpy(r.backward(dL, dL_dalpha=wide[:, ::2], **f["kw"]))
    b = _numpy(r.backward(dL, dL_dalpha=f["t"](f["ga"]), **f["kw"]))
    assert all(np.array_equal(a[k], b[k]) for k in a)
