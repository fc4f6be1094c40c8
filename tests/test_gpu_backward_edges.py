"""GPU: the render backward (csrc/backward.hip, render_backward_kernel) Gaussian by Gaussian at the blend's decision boundaries.

tests/test_gpu_backward.py compares every gradient with one tolerance for the whole frame; where splats overlap, gradients
span orders of magnitude and a Gaussian behind an opaque front could be wrong by 100 % under it. Here every Gaussian of small,
hand-placed scenes is compared with the float64 oracle on its own scale (helpers.assert_backward_per_gaussian): the oracle's
forward is the float32 forward (oracle/backward_np.py f32_forward), so its contributing set is the GPU's bit for bit, and
what is left is the backward's own arithmetic. Each scene asserts that its boundary is really hit:

  a. termination          pixels of one tile ending at different list positions (mid-batch, past 64, past 256), a record
                          that ends one pixel while it is the last contributor of its neighbour; cut-offs 1e-3 and 1e-4
  b. alpha clamp          raw = opacity G crossing 0.99 inside footprints; a Gaussian clamped on every pixel it composites
  c. 1/255                twins: opacity bisected (host expf) so that the brightest pixel's alpha is the smallest float
                          >= 1/255, and the next float below: the first gets gradient, the twin exactly none
  d. long lists           > 300 records per tile, a pixel ended in the fifth 64-entry batch, a frame of 40 x 27 (ragged edges)
  e. a screen-filling     splat (conic condition number ~ 1e6) in front of and behind small ones
  f. garden_like_scene    at two poses
  g. per-entry sums       large splats over a 96 x 80 frame: R >= 6 E, so the block feed's per-entry float sums fit

Every scene runs under the paths that change how the gradients are gathered: the sorted list; the block lists without sorted
lists; float sums as well as double ones; the forward's reordered tiles (tile history, second call: asserted to have been
reordered); one band of tile rows. The block lists take one of two ways to the per-Gaussian sums (csrc/backward.hip,
block_acc_fits): per-entry float sums over the block's tiles, flushed once per entry, where 12 E floats fit in 2 R (E: the
block-list entries, one per visible Gaussian on these one-block frames; R: the instances) — scene g only — or direct atomics
per tile — every other scene. Which one a scene takes is asserted.
"""
import numpy as np
import pytest

from helpers import assert_backward_inputs, assert_backward_per_gaussian, gradients_of, oracle_gradients

pytestmark = pytest.mark.gpu

THRESH = np.float32(1.0 / 255.0)


# ---- scene construction: isotropic (or given) splats placed in pixel space for the default camera -------------------------
def _place(cam, px, py, z):
    """World (X, Y) at world depth z that projects to the pixel centre (px, py) (oracle/backward_np.project_mean2d: affine in X, Y
    at a fixed z for the axis-aligned default camera)."""
    from oracle import backward_np as B
    o = B.project_mean2d(np.array([0.0, 0.0, z]), cam.proj, cam.width, cam.height)
    ex = B.project_mean2d(np.array([1.0, 0.0, z]), cam.proj, cam.width, cam.height) - o
    ey = B.project_mean2d(np.array([0.0, 1.0, z]), cam.proj, cam.width, cam.height) - o
    return np.linalg.solve(np.stack([ex, ey], 1), np.array([px, py]) - o)


def _splats(cam, rows):
    """rows: (px, py, z, sigma_px, opacity, dc[3]) — sigma_px the 3-D scale as pixels at that depth (the 2-D covariance adds 0.3),
    or a (sx, sy) pair with a rotation angle about the view axis: (px, py, z, (sx, sy, angle), opacity, dc)."""
    n = len(rows)
    focal = cam.height / (2.0 * cam.tan_fovy)
    means = np.ones((n, 4), np.float32)
    scales = np.full((n, 4), np.e, np.float32)
    rots = np.zeros((n, 4), np.float32)
    rots[:, 0] = 1.0
    op = np.zeros(n, np.float32)
    shs = np.zeros((n, 48), np.float32)
    for i, (px, py, z, sig, o, dc) in enumerate(rows):
        means[i, :2] = _place(cam, px, py, z)
        means[i, 2] = z
        per_px = (z + 5.0) / focal                      # world units per pixel at depth z (camera at z = -5)
        if np.ndim(sig) == 0:
            scales[i, :3] = max(float(sig), 1e-4) * per_px
        else:
            sx, sy, ang = sig
            scales[i, :3] = (sx * per_px, sy * per_px, 1e-4 * per_px)
            rots[i] = (np.cos(ang / 2), 0.0, 0.0, np.sin(ang / 2))
        op[i] = o
        shs[i, :3] = dc
    return {"means3D": means, "scales": scales, "rotations": rots, "opacities": op, "shs": shs}


def _camera(w, h):
    from gsrast_amd import camera
    return camera.default_camera(w, h, near=0.05, far=50.0)


def _stack_rows(rng, w, h, n_faint, n_front, faint_op=(0.05, 0.12)):
    """An opaque stack: n_front strong splats in front over the left half of every tile column (pixels there end within the
    first batch), then n_faint large faint ones at random depths over the whole frame (pixels elsewhere end hundreds of records
    down the list, at positions that vary from pixel to pixel)."""
    rows = []
    for _ in range(n_front):
        rows.append((16 * rng.integers(0, (w + 15) // 16) + rng.uniform(0, 6), rng.uniform(0, h), rng.uniform(-2.0, -1.5),
                     rng.uniform(1.5, 3.0), rng.uniform(0.6, 0.95), rng.uniform(-1, 1, 3)))
    for _ in range(n_faint):
        rows.append((rng.uniform(-4, w + 4), rng.uniform(-4, h + 4), rng.uniform(-1.0, 1.0), rng.uniform(4.0, 10.0),
                     rng.uniform(*faint_op), rng.uniform(-1, 1, 3)))
    return rows


def _ring_rows(cx, cy, centre_op):
    """A tiny splat (2-D conic ~ 3.33: only the centre pixel and its eight neighbours can reach 1/255) at opacity `centre_op`
    centred on pixel (cx, cy), BEHIND two nearly opaque tiny splats on each of the eight neighbours: those end the neighbours
    before the list reaches the centre splat, so the only pixel that composites it is its centre, where raw > 0.99."""
    rows = []
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                for z in (-1.2, -1.1):
                    rows.append((cx + dx, cy + dy, z + 0.01 * (dx + 3 * dy), 0.0, 0.999, (0.8, -0.3, 0.4)))
    rows.append((cx, cy, 0.5, 0.0, centre_op, (0.2, 0.9, -0.5)))
    return rows


def _twin_opacities(scene, cam, pairs):
    """Bisects the opacity of each (first, twin) pair of rows with the host expf: first — the smallest float32 opacity for which
    the brightest pixel's alpha = opacity G (the forward's float32 power and exp) reaches 1/255; twin — the float below."""
    from oracle import cpu_oracle
    st = cpu_oracle.forward(scene, cam)
    f = np.float32
    ys, xs = np.mgrid[0:cam.height, 0:cam.width]
    for a, b in pairs:
        for i in (a, b):
            xy, co = st["means2D"][i], st["conicOpacity"][i]
            dx, dy = f(xy[0]) - xs.astype(f), f(xy[1]) - ys.astype(f)
            power = f(-0.5) * ((co[0] * dx) * dx + (co[2] * dy) * dy) - (co[1] * dx) * dy
            G = cpu_oracle.expf(np.minimum(power, f(0.0))).reshape(power.shape)[power <= 0]
            lo, hi = np.float32(1e-3).view(np.uint32), np.float32(1.0).view(np.uint32)
            while lo < hi:                                       # smallest op with max fl(op G) >= 1/255
                mid = np.uint32((int(lo) + int(hi)) // 2)
                if (mid.view(np.float32) * G >= THRESH).any():
                    hi = mid
                else:
                    lo = np.uint32(mid + 1)
            op = lo.view(np.float32)
            scene["opacities"][i] = op if i == a else np.nextafter(op, f(0.0))
    return scene


def _twin_rows():
    """Pairs of faint tiny splats (first, twin: consecutive rows) centred on a pixel, and off the grid by (0.5, 0.5), (0.5, 0)
    and (0.3, 0.2): one to four pixels at the brightest alpha."""
    rows = []
    for j, (ox, oy) in enumerate(((0.0, 0.0), (0.5, 0.5), (0.5, 0.0), (0.3, 0.2))):
        rows.append((5 + 11 * j + ox, 8 + oy, 0.1 * j, 0.0, 0.01, (0.5, 0.2, -0.4)))
        rows.append((5 + 11 * j + ox, 30 + oy, 0.1 * j + 0.05, 0.0, 0.01, (-0.3, 0.6, 0.1)))
    return rows


# ---- the scenes -------------------------------------------------------------------------------------------------------------
def scene_termination(rng_seed=1):
    w, h = 48, 32
    cam = _camera(w, h)
    rows = _stack_rows(np.random.default_rng(rng_seed), w, h, n_faint=420, n_front=150, faint_op=(0.06, 0.14))
    return _splats(cam, rows), cam


def scene_clamp():
    w, h = 48, 32
    cam = _camera(w, h)
    rows = _ring_rows(8, 8, 1.0) + _ring_rows(8, 22, 0.995)
    rng = np.random.default_rng(4)
    for _ in range(8):                                 # larger splats whose raw crosses 0.99 inside the footprint
        rows.append((rng.uniform(20, 44), rng.uniform(4, 28), rng.uniform(-1, 1), rng.uniform(1.5, 4.0), rng.uniform(0.995, 1.0),
                     rng.uniform(-1, 1, 3)))
    return _splats(cam, rows), cam


def scene_twins():
    w, h = 48, 48
    cam = _camera(w, h)
    rows = _twin_rows()
    scene = _splats(cam, rows)
    pairs = [(i, i + 1) for i in range(0, len(rows), 2)]
    return _twin_opacities(scene, cam, pairs), cam


def scene_long_lists():
    w, h = 40, 27
    cam = _camera(w, h)
    rows = _stack_rows(np.random.default_rng(5), w, h, n_faint=520, n_front=100)
    return _splats(cam, rows), cam


def scene_screen_filling(front):
    w, h = 64, 48
    cam = _camera(w, h)
    rng = np.random.default_rng(6)
    rows = [(rng.uniform(0, w), rng.uniform(0, h), rng.uniform(-0.5, 0.5), rng.uniform(0.5, 3.0), rng.uniform(0.2, 0.9),
             rng.uniform(-1, 1, 3)) for _ in range(60)]
    rows.insert(7, (w / 2 + 0.3, h / 2 - 0.2, -1.5 if front else 1.5, (3000.0, 3.0, 0.35), 0.7, (0.6, -0.2, 0.3)))
    return _splats(cam, rows), cam


def scene_per_entry_sums():
    w, h = 96, 80
    cam = _camera(w, h)
    rng = np.random.default_rng(8)
    rows = [(rng.uniform(-8, w + 8), rng.uniform(-8, h + 8), rng.uniform(-1.0, 1.0), rng.uniform(6.0, 14.0), rng.uniform(0.05, 0.6),
             rng.uniform(-1, 1, 3)) for _ in range(220)]
    return _splats(cam, rows), cam


def scene_garden(pose):
    from gsrast_amd import camera, scenes
    w, h = 96, 64
    scene = scenes.garden_like_scene(3000, seed=21)
    scene["means3D"][:, :3] *= 0.25
    pos = (0.0, 0.0, -5.0) if pose == 0 else (0.4, -0.3, -4.0)
    return scene, camera.default_camera(w, h, near=0.05, far=50.0, position=pos)


# ---- what each scene must really exercise (asserted on the oracle's evaluation of the GPU's forward state) -----------------
def _edge_termination(ref, w, h, deep=256):
    nc, stop = ref["n_contrib"], ref["stop_idx"]
    for ty in range((h + 15) // 16):
        for tx in range((w + 15) // 16):
            s = stop[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
            ended = s[s >= 0]
            # one tile whose pixels end mid-batch, past 64 and past `deep`
            if ended.size and (ended % 64 != 63).any() and (ended < 64).any() and (ended >= 64).any() and (ended >= deep).any():
                break
        else:
            continue
        break
    else:
        pytest.fail(f"no tile has pixels ended before 64, past 64 and past {deep}: {np.unique(stop)}")
    # a record that ends a pixel while it is the last contributor of the neighbouring pixel (same tile: same list)
    found = False
    for y in range(h):
        for x in range(w):
            if stop[y, x] < 0:
                continue
            for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                if 0 <= yy < h and 0 <= xx < w and yy // 16 == y // 16 and xx // 16 == x // 16 and nc[yy, xx] == stop[y, x] + 1:
                    found = True
    assert found, "no record ends one pixel while being its neighbour's last contributor"
    return int(stop.max())


def _edge_clamp(ref):
    clamped = (ref["pixels"] > 0) & (ref["free_pixels"] == 0)
    assert clamped.sum() >= 2, "no Gaussian clamped on every pixel it composites"
    crossing = (ref["free_pixels"] > 0) & (ref["free_pixels"] < ref["pixels"])
    assert crossing.any(), "no footprint where raw crosses 0.99"
    return int(clamped.sum())


def _edge_twins(ref, n_pairs):
    for p in range(n_pairs):
        first, twin = 2 * p, 2 * p + 1
        assert 1 <= ref["pixels"][first] <= 4, (p, ref["pixels"][first])
        assert ref["pixels"][twin] == 0, (p, ref["pixels"][twin])
    assert (ref["pixels"][0:2 * n_pairs:2] > 1).any()         # off the grid: more than one pixel passes
    return n_pairs


def _edge_screen_filling(r, idx=7):
    co = r.map_geometry_state()["conicOpacity"][idx].cpu().numpy().astype(np.float64)
    ev = np.linalg.eigvalsh(np.array([[co[0], co[1]], [co[1], co[2]]]))
    cond = ev.max() / ev.min()
    assert cond > 1e5, cond
    return cond


# ---- the run ------------------------------------------------------------------------------------------------------------------
_VARIANTS = (("sorted list", dict(plan="sort"), True),
             ("sorted list, float sums", dict(plan="sort"), False),
             ("block lists", dict(plan="blocks", sorted_lists=False), True),
             ("block lists, float sums", dict(plan="blocks", sorted_lists=False), False),
             ("reordered tiles", dict(plan="sort", tile_history=True), True),
             ("band of tile rows", dict(plan="sort"), True))

SCENES = {
    "termination": (lambda: scene_termination(), "gscuda"),
    "termination, cut-off 1e-4": (lambda: scene_termination(), "inria"),
    "clamp": (scene_clamp, "gscuda"),
    "1/255 twins": (scene_twins, "gscuda"),
    "long lists, ragged frame": (scene_long_lists, "gscuda"),
    "screen-filling splat in front": (lambda: scene_screen_filling(True), "gscuda"),
    "screen-filling splat behind": (lambda: scene_screen_filling(False), "gscuda"),
    "garden, pose 0": (lambda: scene_garden(0), "gscuda"),
    "garden, pose 1": (lambda: scene_garden(1), "gscuda"),
    "per-entry sums": (scene_per_entry_sums, "gscuda"),
}


@pytest.mark.parametrize("name", list(SCENES))
def test_backward_per_gaussian_at_the_edges(name):
    import torch
    from gsrast_amd.rasterizer import SplatRasterizer
    build, semantics = SCENES[name]
    scene, cam = build()
    W, H = cam.width, cam.height
    gx, gy = (W + 15) // 16, (H + 15) // 16
    bg = (0.3, 0.1, 0.6)
    cutoff = 1e-4 if semantics == "inria" else 1e-3
    kw = dict(semantics=semantics, sh_degree=0)
    r = SplatRasterizer(W, H, background=bg)
    r.configure_from_scene(scene)
    n = r.num_gaussians
    dL = torch.randn((3, H, W), generator=torch.Generator().manual_seed(17)).cuda()
    r.draw(cam, plan="sort", tile_history=False, **kw)
    assert r.last_num_rendered > 0
    all_tiles = [(tx, ty) for ty in range(gy) for tx in range(gx)]
    targets = np.arange(n)
    ref = oracle_gradients(r, dL, bg, all_tiles, targets, 4096, f32_forward=True, magnitudes=True, t_cutoff=cutoff, full_lists=True)
    im = r.map_image_state()
    assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), ref, name)
    band = (gy // 2, gy) if gy > 1 else (0, 1)
    ref_band = oracle_gradients(r, dL, bg, [(tx, ty) for tx, ty in all_tiles if band[0] <= ty < band[1]], targets, 4096,
                                f32_forward=True, magnitudes=True, t_cutoff=cutoff, full_lists=True)
    # the boundary of the scene is hit
    if name.startswith("termination"):
        edge = _edge_termination(ref, W, H)
    elif name.startswith("long lists"):
        edge = _edge_termination(ref, W, H)
        assert ((ref["stop_idx"] >= 256) & (ref["stop_idx"] < 320)).any(), "no pixel ended in the fifth batch"
        lengths = np.diff(r.map_image_state()["ranges"].cpu().numpy().view(np.uint32).astype(np.int64), axis=1)
        assert lengths.max() > 300
        # the last tile row and column (partial tiles) composite and are compared
        assert (ref["n_contrib"][-1, :] > 0).all() and (ref["n_contrib"][:, -1] > 0).all()
    elif name == "clamp":
        edge = _edge_clamp(ref)
    elif name == "1/255 twins":
        edge = _edge_twins(ref, n // 2)
    elif name.startswith("screen-filling"):
        edge = _edge_screen_filling(r)
        assert ref["tiles"][7] >= (3 * gx * gy) // 4
    else:
        edge = int((ref["pixels"] > 0).sum())
        assert edge >= 100
    # which way the block lists take to the per-Gaussian sums: per-entry sums where 12 E floats fit in the 2 R of scratch
    # and the forward blend looked into at most two units of the block's list (api.hip block feed, backward.hip block_acc_fits;
    # one block of 8 x 8 tiles holds the whole frame, so E = the Gaussians that touch a tile)
    assert gx <= 8 and gy <= 8
    E = int((r.map_geometry_state()["tilesTouched"] > 0).sum())
    R = r.last_num_rendered
    per_entry = 6 * E <= R and E <= 2 * 2048
    assert per_entry == (name == "per-entry sums"), (name, R, E)
    print(f"[edges] {name}: N={n}, R={r.last_num_rendered}, deepest last contributor {int(ref['n_contrib'].max())}, edge {edge}")

    worst = {}
    for vname, dkw, wide in _VARIANTS:
        rows = band if vname.startswith("band") else None
        if vname == "reordered tiles":
            r.draw(cam, **dkw, **kw)                    # the first call fills the history; the second is reordered by it
        r.draw(cam, tile_rows=rows, **({"tile_history": False} | dkw), **kw)
        if vname == "reordered tiles":
            assert r.last_tiles_reordered and not r.last_tile_order_dropped, name
        blocks = dkw["plan"] == "blocks"
        if blocks:
            assert r.last_plan == "blocks" and not r.last_lists_written and not r.last_blend_from_lists
        use = ref_band if rows else ref
        im = r.map_image_state()
        assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), use, f"{name}, {vname}")
        got = r.backward(dL, tile_rows=rows, wide_sums=wide, **kw)
        # (per-entry sums are float sums over up to 64 tiles whatever wide_sums says: the bound's tiles term applies)
        worst[vname] = assert_backward_per_gaussian(gradients_of(got, targets), use, float_tile_sums=not wide or (blocks and per_entry),
                                                    what=f"{name}, {vname}")
    print(f"[edges] {name}: worst ratios " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
