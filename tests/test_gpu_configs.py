"""GPU: BASELINE.json configs 3, 4 and 5 at their workloads (the path of reference GSCuda.cu:695-811).

  config 3  5 834 784 splats (garden-like stand-in, seed 43) at 3840 x 2160, tile rows in 8 uneven bands:
            the banded frame equals the whole frame bit for bit; every 8th splat at 4K against the CPU oracle.
  config 4  50 M anisotropic splats (seed 44) at 1920 x 1080: both binning plans bit-equal, list properties,
            every 16th splat against the CPU oracle (per-Gaussian outputs of the full run too).
  config 5  forward + backward on the 5.83 M-splat scene at 1920 x 1080: finite everywhere, zero for culled
            splats, Gaussians picked at random checked against oracle/backward_np.py on the tiles they touch.

The scenes are generated on the device (gsrast_amd/scenes.py: same splitmix64 definition); the oracle's inputs
are copied FROM the device scene so both sides see the same bits.
"""
import gc

import numpy as np
import pytest

from helpers import assert_blend_parity, check_backward_chain, gradients_of, image_report, oracle_gradients

pytestmark = pytest.mark.gpu


def _release():
    import torch
    gc.collect()
    torch.cuda.empty_cache()


def _threads():
    from oracle import cpu_oracle
    return max(1, min(64, cpu_oracle.hardware_concurrency()))


def _compare_with_oracle(r, exp, img, what):
    """Lists, per-Gaussian floats, transmittance and nContrib bit for bit; pixels within 2e-6 (north star: 1e-4)."""
    assert r.last_num_rendered == exp["num_rendered"], what
    assert r.last_records_staged == exp["records_staged"], what
    g = r.map_geometry_state()
    vis = exp["tilesTouched"] > 0               # (the per-Gaussian arrays are only written for visible Gaussians)
    for k in ("means2D", "depths", "cov3D", "rgb", "conicOpacity"):
        assert np.array_equal(g[k].cpu().numpy()[vis], exp[k][vis]), (what, k)
    assert np.array_equal(g["radii"].cpu().numpy(), exp["radii"]), what
    assert np.array_equal(g["tilesTouched"].cpu().numpy().view(np.uint32), exp["tilesTouched"]), what
    b = r.map_binning_state()
    assert np.array_equal(b["keys"].cpu().numpy().view(np.uint64), exp["keys"]), what
    assert np.array_equal(b["values"].cpu().numpy().view(np.uint32), exp["values"]), what
    assert np.array_equal(r.map_image_state()["ranges"].cpu().numpy().view(np.uint32), exp["ranges"]), what
    im = r.map_image_state()
    max_err = assert_blend_parity(img, im["finalT"].cpu().numpy(), im["nContrib"].cpu().numpy(), exp,
                                  f"{what}: R={r.last_num_rendered} R_f={r.last_records_staged} plan={r.last_plan}")
    return max_err


def test_config3_garden_4k_in_eight_bands_and_against_the_oracle():
    import torch
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    from oracle import cpu_oracle
    W, H = 3840, 2160
    scene = scenes.garden_like_scene_device(5_834_784, seed=43, device="cuda:0")
    pos = scene["means3D"][:, :3]
    span = float((pos.max(0).values - pos.min(0).values).max())
    cam = camera.default_camera(W, H, near=0.001 * span, far=span)
    r = SplatRasterizer(W, H, background=(0.0, 0.0, 0.0))
    r.configure_from_scene(scene)
    img = r.draw(cam).clone()
    R = r.last_num_rendered
    assert R > 1_000_000_000 and r.last_plan == "blocks"          # 1.2 G instances: 28 % of the 32-bit offset range
    b = r.map_binning_state()
    assert bool((b["keys"][1:] >= b["keys"][:-1]).all()), "sorted keys out of order"
    rg = r.map_image_state()["ranges"].to(torch.int64)
    assert int((rg[:, 1] - rg[:, 0]).sum()) == R
    # tile rows in 8 uneven bands, as 8 ranks would hold them (135 tile rows)
    bands = ((0, 11), (11, 30), (30, 47), (47, 64), (64, 70), (70, 95), (95, 118), (118, 135))
    r.out_color.fill_(-1.0)
    total = 0
    for rows in bands:
        r.draw(cam, tile_rows=rows)
        total += r.last_num_rendered
    assert total == R, "bands must partition the instances"
    assert torch.equal(r.out_color, img), "banded 4K frame differs from the whole frame"
    r = b = rg = img = None
    _release()

    # every 8th splat at the same camera and resolution against the CPU oracle (R of the sample ~ 150 M)
    sub = scenes.scene_rows(scene, slice(None, None, 8))
    del scene
    exp = cpu_oracle.forward(sub, cam, (0.0, 0.0, 0.0), threads=_threads())
    r2 = SplatRasterizer(W, H, background=(0.0, 0.0, 0.0))
    r2.configure_from_scene(sub)
    img2 = r2.draw(cam, count_staged=True).cpu().numpy()
    assert exp["num_rendered"] > 100_000_000
    _compare_with_oracle(r2, exp, img2, "config 3, every 8th splat at 4K")


def test_config4_50m_stress_plans_agree_and_sample_against_the_oracle():
    import torch
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    from oracle import cpu_oracle
    W, H, N = 1920, 1080, 50_000_000
    scene = scenes.stress_scene_device(N, seed=44, device="cuda:0")          # gscuda semantics read the DC triple only
    cam = camera.default_camera(W, H, near=0.1, far=100.0, position=(0.0, 0.0, -25.0))
    r = SplatRasterizer(W, H, background=(0.0, 0.0, 0.0))
    r.configure_from_scene(scene)
    img_auto = r.draw(cam, count_staged=True).clone()
    staged = r.last_records_staged
    assert r.last_plan == "sort"                                              # R / N = 2.5: below the block plan's threshold
    R = r.last_num_rendered
    assert R > 100_000_000
    b = r.map_binning_state()
    keys_s, vals_s = b["keys"].clone(), b["values"].clone()
    ranges_s = r.map_image_state()["ranges"].clone()
    img_b = r.draw(cam, plan="blocks", count_staged=True)
    assert r.last_plan == "blocks" and r.last_num_rendered == R and r.last_records_staged == staged
    b = r.map_binning_state()
    assert torch.equal(b["keys"], keys_s) and torch.equal(b["values"], vals_s), "the two binning plans differ"
    assert torch.equal(r.map_image_state()["ranges"], ranges_s)
    assert torch.equal(img_b, img_auto)
    # list properties (no oracle needed): sorted, ties by index, depth half = depth of the Gaussian, ranges partition
    g = r.map_geometry_state()
    tt = g["tilesTouched"].to(torch.int64) & 0xFFFFFFFF
    assert int(tt.sum()) == R == (int(g["pointOffsets"][-1]) & 0xFFFFFFFF)
    assert bool((keys_s[1:] >= keys_s[:-1]).all())
    tie = keys_s[1:] == keys_s[:-1]
    assert bool((vals_s[1:][tie] > vals_s[:-1][tie]).all())
    depth_bits = g["depths"].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    samp = torch.randint(0, R, (2_000_000,), device=keys_s.device, generator=torch.Generator(device=keys_s.device).manual_seed(1))
    assert bool(((keys_s[samp] & 0xFFFFFFFF) == depth_bits[vals_s[samp].to(torch.int64)]).all())
    counts = torch.bincount(keys_s >> 32, minlength=120 * 68)
    rg = ranges_s.to(torch.int64)
    assert bool(((rg[:, 1] - rg[:, 0]) == counts).all())
    del keys_s, vals_s, tie, samp, counts, depth_bits

    # every 16th splat: the full run's per-Gaussian outputs at those rows, then the sample rendered on its own
    rows = slice(None, None, 16)
    sub = scenes.scene_rows(scene, rows)
    exp = cpu_oracle.forward(sub, cam, (0.0, 0.0, 0.0), threads=_threads())
    vis = exp["tilesTouched"] > 0
    assert vis.sum() > 1_000_000
    for k in ("means2D", "depths", "cov3D", "rgb", "conicOpacity"):
        assert np.array_equal(g[k][rows].cpu().numpy()[vis], exp[k][vis]), k
    assert np.array_equal(g["radii"][rows].cpu().numpy(), exp["radii"])
    assert np.array_equal(g["tilesTouched"][rows].cpu().numpy().view(np.uint32), exp["tilesTouched"])
    del g, b, rg, img_auto, img_b
    r = None
    del scene
    _release()
    for plan in ("sort", "blocks"):
        r2 = SplatRasterizer(W, H, background=(0.0, 0.0, 0.0))
        r2.configure_from_scene(sub)
        img2 = r2.draw(cam, count_staged=True, plan=plan).cpu().numpy()
        assert r2.last_plan == plan
        _compare_with_oracle(r2, exp, img2, f"config 4, every 16th splat, plan {plan}")
        r2 = None
        _release()


def test_config4_as_written_sh_degree3_under_the_upstream_profile():
    """BASELINE config 4 as written ("50M synthetic anisotropic Gaussians, SH deg 3"): the reference's own semantics read
    the DC triple only, so degree 3 means the upstream profile (GSR_FLAG_SEMANTICS_INRIA). Parity unpinned (no upstream
    source in the tree): the checker is oracle/inria_np.py. The per-Gaussian stage is what this configuration adds — 48 SH
    floats per Gaussian through the degree-3 basis — and it is compared at every 64th row of the full run; binning and
    blend are the kernels the other tests cover, checked here by the two plans agreeing and by the list properties."""
    import torch
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    from oracle import inria_np
    W, H, N = 1920, 1080, 50_000_000
    scene = scenes.stress_scene_device(N, seed=44, device="cuda:0", full_sh=True)       # 9.6 GB of SH coefficients
    cam = camera.default_camera(W, H, near=0.1, far=100.0, position=(0.0, 0.0, -25.0))
    r = SplatRasterizer(W, H, background=(0.1, 0.2, 0.3))
    r.configure_from_scene(scene)
    img = r.draw(cam, semantics="inria", sh_degree=3).clone()
    R = r.last_num_rendered
    assert R > 50_000_000 and r.last_plan == "sort"
    g = r.map_geometry_state()
    rows = slice(None, None, 64)
    sub = scenes.scene_rows(scene, rows)
    exp = inria_np.preprocess(sub, cam, 3)
    vis = exp["tilesTouched"] > 0
    assert vis.sum() > 500_000
    assert np.array_equal(g["radii"][rows].cpu().numpy(), exp["radii"])
    assert np.array_equal(g["tilesTouched"][rows].cpu().numpy().view(np.uint32), exp["tilesTouched"])
    for k in ("means2D", "depths", "conicOpacity"):
        assert np.array_equal(g[k][rows].cpu().numpy()[vis], exp[k][vis]), k
    rgb = g["rgb"][rows].cpu().numpy()[vis]
    assert np.array_equal(rgb.view(np.uint32), exp["rgb"][vis].view(np.uint32))    # the same float32 expression, left to right, no contraction
    assert rgb.min() >= 0.0 and (rgb == 0.0).mean() > 0.01                   # the clamp at zero is exercised
    tt = g["tilesTouched"].to(torch.int64) & 0xFFFFFFFF
    assert int(tt.sum()) == R
    b = r.map_binning_state()
    keys, vals = b["keys"].clone(), b["values"].clone()
    assert bool((keys[1:] >= keys[:-1]).all())
    tie = keys[1:] == keys[:-1]
    assert bool((vals[1:][tie] > vals[:-1][tie]).all())
    depth_bits = g["depths"].view(torch.int32).to(torch.int64) & 0xFFFFFFFF         # view-space z is the key here
    samp = torch.randint(0, R, (1_000_000,), device=keys.device, generator=torch.Generator(device=keys.device).manual_seed(2))
    assert bool(((keys[samp] & 0xFFFFFFFF) == depth_bits[vals[samp].to(torch.int64)]).all())
    del tie, samp, depth_bits, tt
    img_b = r.draw(cam, semantics="inria", sh_degree=3, plan="blocks")
    assert r.last_plan == "blocks" and r.last_num_rendered == R
    b = r.map_binning_state()
    assert torch.equal(b["keys"], keys) and torch.equal(b["values"], vals) and torch.equal(img_b, img)
    # a lower degree gives a different image: the higher bands are really evaluated
    img1 = r.draw(cam, semantics="inria", sh_degree=1)
    assert float((img1 - img).abs().max()) > 1e-2


def _tile_rects(means2D, ext, gx, gy):
    """getRect (GSCuda.cu:248-259) with the stored extents, in torch float32: [x0, x1) x [y0, y1) in tiles."""
    import torch
    p = means2D
    e = ext.to(torch.float32)
    x0 = ((p[:, 0] - e[:, 0]) / 16.0).to(torch.int32).clamp(0, gx)
    y0 = ((p[:, 1] - e[:, 1]) / 16.0).to(torch.int32).clamp(0, gy)
    x1 = ((((p[:, 0] + e[:, 0]) + 16.0) - 1.0) / 16.0).to(torch.int32).clamp(0, gx)     # operation order of the kernel
    y1 = ((((p[:, 1] + e[:, 1]) + 16.0) - 1.0) / 16.0).to(torch.int32).clamp(0, gy)
    return x0, y0, x1, y1


def _compare_gradients(got_dev, targets, exp, allowed_outliers, what):
    got = gradients_of(got_dev, targets)
    for k in exp:
        scale = max(1e-6, float(np.abs(exp[k]).max()))
        err = np.abs(got[k] - exp[k]).max(1)
        # float32 atomics in varying order against a float64 sum: 2e-4 of the largest gradient; a threshold flip on a
        # pixel (counted by the caller) may move one Gaussian further
        assert int((err > 2e-4 * scale).sum()) <= allowed_outliers, (what, k, float(err.max()), scale)
        zero = np.abs(exp[k]).sum(1) == 0
        if allowed_outliers == 0:
            assert (got[k][zero] == 0).all(), (what, k, "a Gaussian no pixel composites must get exactly zero")


def _check_pose(r, scene, cam, bg, seed, min_with_gradient, n_windows=40, max_tiles_each=64, max_union=700, max_pick=120,
                max_depth=6000, most_tiles=0):
    # max_depth: the oracle holds [records x 256] float64 arrays per tile; tiles whose deepest pixel walks more are passed over
    """forward + backward at one camera; returns the number of Gaussians that received colour gradient."""
    import torch
    from gsrast_amd import scenes
    W, H = r.width, r.height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r.draw(cam)
    dL = torch.randn((3, H, W), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(seed))
    got_dev = r.backward(dL)
    geo = r.map_geometry_state()
    culled = geo["radii"] <= 0
    for k, v in got_dev.items():
        assert bool(torch.isfinite(v).all()), k
        assert bool((v[culled] == 0).all()), (k, "culled splats must get zero gradient")
    with_grad = got_dev["dL_dcolors"].abs().sum(1) > 0
    x0, y0, x1, y1 = _tile_rects(geo["means2D"], r.rects, gx, gy)
    tt = geo["tilesTouched"].to(torch.int64)
    vis = tt > 0
    assert bool((((x1 - x0) * (y1 - y0)).to(torch.int64)[vis] == tt[vis]).all())
    nc = r.map_image_state()["nContrib"].to(torch.int32)
    tile_depth = torch.nn.functional.pad(nc, (0, gx * 16 - W, 0, gy * 16 - H)).view(gy, 16, gx, 16).amax(dim=(1, 3))
    deep = (tile_depth > max_depth).cpu().numpy()

    # (1) Gaussians chosen at random among those whose tiles all lie inside one of 40 random 2 x 2-tile windows: their
    # gradients come from those tiles only, so the oracle evaluated on the windows gives them completely.
    rng = np.random.default_rng(seed)
    wins = []
    for _ in range(1000):
        wx, wy = int(rng.integers(0, gx - 1)), int(rng.integers(0, gy - 1))
        if (wx, wy) not in wins and not deep[wy:wy + 2, wx:wx + 2].any():
            wins.append((wx, wy))
        if len(wins) == n_windows:
            break
    assert len(wins) >= n_windows // 2, len(wins)
    inside = torch.zeros_like(vis)
    for wx, wy in wins:
        inside |= vis & (x0 >= wx) & (x1 <= wx + 2) & (y0 >= wy) & (y1 <= wy + 2)
    # up to 1 000 of those that received gradient and up to 1 000 of those that did not (on a frame whose tiles saturate
    # early, a uniform draw among the visible Gaussians would hold almost none of the former)
    pool_a = torch.nonzero(inside & with_grad).flatten().cpu().numpy()
    pool_b = torch.nonzero(inside & ~with_grad).flatten().cpu().numpy()
    pick = np.random.default_rng(seed + 1)
    cand = np.sort(np.concatenate([pick.permutation(pool_a)[:1000], pick.permutation(pool_b)[:1000]]))
    assert cand.size >= 500, (pool_a.size, pool_b.size)
    tiles = sorted({(wx + i, wy + j) for wx, wy in wins for i in (0, 1) for j in (0, 1)})
    ref = oracle_gradients(r, dL, bg, tiles, cand, max_depth)
    exp, mismatch = ref["exp"], len(ref["differs"])
    assert mismatch <= 8, mismatch              # exp implementations may flip a threshold on a handful of pixels
    _compare_gradients(got_dev, cand, exp, mismatch, "random Gaussians inside windows")
    n_grad = int((np.abs(exp["dL_dcolors"]).sum(1) > 0).sum())
    assert n_grad >= min_with_gradient, n_grad

    # (2) Gaussians that DID receive gradient, the ones touching the fewest tiles first (their tiles not deeper than the cap)
    gid = torch.nonzero(with_grad & (tt <= max_tiles_each)).flatten()
    gid = gid[torch.argsort(tt[gid])][:400].cpu().numpy()
    keep, tiles = [], set()
    hx0, hy0, hx1, hy1 = (v.cpu().numpy() for v in (x0, y0, x1, y1))
    for i in gid:
        mine = {(tx, ty) for ty in range(hy0[i], hy1[i]) for tx in range(hx0[i], hx1[i])}
        if any(deep[ty, tx] for tx, ty in mine) or len(tiles | mine) > max_union:
            continue
        keep.append(int(i))
        tiles |= mine
        if len(keep) == max_pick:
            break
    keep = np.asarray(sorted(keep))
    if keep.size:
        ref2 = oracle_gradients(r, dL, bg, sorted(tiles), keep, max_depth)
        exp2, mismatch2 = ref2["exp"], len(ref2["differs"])
        assert mismatch2 <= 8, mismatch2
        _compare_gradients(got_dev, keep, exp2, mismatch2, "Gaussians with gradient")
        assert (np.abs(exp2["dL_dcolors"]).sum(1) > 0).all()
        # the chain to the inputs for those
        sel = torch.from_numpy(keep).to("cuda:0")
        host_scene = scenes.scene_rows(scene, sel)
        full = {k: got_dev[k][sel].cpu().numpy() for k in
                ("dL_dconic_opacity", "dL_dmean2D", "dL_dcov2D", "dL_dcov3D", "dL_dmeans3D", "dL_dscales", "dL_drotations")}
        mags = check_backward_chain(full, {"cov3D": geo["cov3D"][sel].cpu().numpy()}, host_scene, cam, W, H, np.arange(keep.size))
        assert all(m > 0 for m in mags)
    # (3) the splats that HURT: the Gaussians with gradient that touch the most tiles — screen-filling, a few centimetres from
    # the camera, conics with a condition number of 1e6. Every tile of the frame is evaluated by the float64 oracle (frames of
    # shallow tiles only: `most_tiles` is set for the pose inside the cloud) and the chain is checked END TO END against the
    # oracle's own sums, at 1e-3 of each Gaussian's own largest component.
    if most_tiles:
        assert not deep.any()
        gid = torch.nonzero(with_grad).flatten()
        big = gid[torch.argsort(tt[gid], descending=True)][:most_tiles].cpu().numpy()
        big = np.asarray(sorted(int(i) for i in big))
        all_tiles = [(tx, ty) for ty in range(gy) for tx in range(gx)]
        bad_px = []
        # (the oracle's forward in float32, as the HIP forward computes it: the backward of one and the same function)
        exp3 = oracle_gradients(r, dL, bg, all_tiles, big, max_depth, bad_pixels=bad_px, f32_forward=True)["exp"]
        assert len(bad_px) <= 8, len(bad_px)
        if bad_px:
            # The two forwards disagree on a few pixels that sit on a hard threshold; a Gaussian whose sum over two million
            # pixels nearly cancels sees such a pixel in its third digit. Those pixels are taken out of the loss on BOTH sides:
            # what is compared is the backward of one and the same forward.
            dL = dL.clone()
            ys, xs = (torch.tensor(v, device=dL.device) for v in zip(*bad_px))
            sub = sorted({(x // 16, y // 16) for y, x in bad_px})
            before = oracle_gradients(r, dL, bg, sub, big, max_depth, f32_forward=True)["exp"]
            dL[:, ys, xs] = 0.0
            after = oracle_gradients(r, dL, bg, sub, big, max_depth, f32_forward=True)["exp"]
            exp3 = {k: exp3[k] - before[k] + after[k] for k in exp3}
            got_dev = r.backward(dL)
        sel = torch.from_numpy(big).to("cuda:0")
        got3 = {k: got_dev[k][sel].cpu().numpy() for k in
                ("dL_dconic_opacity", "dL_dmean2D", "dL_dcov2D", "dL_dcov3D", "dL_dmeans3D", "dL_dscales", "dL_drotations")}
        for k, idx3 in (("dL_dcov2D", slice(0, 3)), ("dL_dmean2D", slice(0, 2))):
            e, gv = exp3[k], got3[k][:, idx3]
            err = np.abs(gv - e).max(1) / np.maximum(np.abs(e).max(1), 1e-30)
            print(f"[backward] {most_tiles} Gaussians with the most tiles ({int(tt[sel].min())}-{int(tt[sel].max())} tiles): {k} worst relative error {err.max():.2e}")
            assert (err <= 1e-3).all(), (k, float(err.max()))
        up = {"dL_dconic_opacity": np.concatenate([exp3["dL_dconic"], exp3["dL_dopacity"]], 1), "dL_dmean2D": exp3["dL_dmean2D"],
              "dL_dcov2D": exp3["dL_dcov2D"]}
        check_backward_chain(got3, {"cov3D": geo["cov3D"][sel].cpu().numpy()}, scenes.scene_rows(scene, sel), cam, W, H,
                             np.arange(big.size), upstream=up, tol_scale=1.0 / 3.0)      # 0.7e-3 / 1e-3 of the Gaussian's own largest component
    return int(with_grad.sum()), int(keep.size)


def test_config5_garden_1080p_forward_backward_fullsize():
    from gsrast_amd import camera, scenes
    from gsrast_amd.rasterizer import SplatRasterizer
    W, H, N = 1920, 1080, 5_834_784
    scene = scenes.garden_like_scene_device(N, seed=43, device="cuda:0")
    pos = scene["means3D"][:, :3]
    span = float((pos.max(0).values - pos.min(0).values).max())
    bg = (0.1, 0.3, 0.2)
    r = SplatRasterizer(W, H, background=bg)
    r.configure_from_scene(scene)
    # the reference's default pose (BENCH frame): the camera sits inside the cloud, a few near splats saturate every
    # tile, so about a thousand Gaussians receive gradient at all
    cam = camera.default_camera(W, H, near=0.001 * span, far=span)
    # (those are large: the ones checked in full touch up to 1 200 tiles each)
    n_grad, n_checked = _check_pose(r, scene, cam, bg, seed=7, min_with_gradient=0, max_tiles_each=1200, max_union=1500, max_pick=40,
                                    most_tiles=20)
    assert r.last_num_rendered > 200_000_000 and n_grad > 500 and n_checked >= 5, (n_grad, n_checked)
    # a pose outside the cloud: small splats, deep lists, most visible Gaussians receive gradient
    cam2 = camera.default_camera(W, H, near=0.001 * span, far=span, position=(0.0, 0.0, -14.0))
    n_grad2, n_checked2 = _check_pose(r, scene, cam2, bg, seed=9, min_with_gradient=100, n_windows=24, max_depth=10000)
    assert n_grad2 > 100_000 and n_checked2 >= 20, (n_grad2, n_checked2)
