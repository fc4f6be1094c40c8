"""CPU: the replay and the back walk that the references of the list-walk passes share (tests/walk_ref.py), pinned directly to
the two anchors kept apart from it: the replay's finalT / nContrib to the C++ oracle's (cpu_oracle.forward, and blend_cutoff for
the upstream profile's cut-off) bit for bit, the tile decisions to that replay, and the geometry sums and their condition scales
of a three-channel colour term to oracle/backward_np.blend_tile_backward — so that a pass's reference can stand on walk_ref.py
without going through another pass's tests."""
import functools

import numpy as np
import pytest

import absgrad_ref as A
import walk_ref as R
from oracle import backward_np as B
from oracle import cpu_oracle

SCENES = {name: (scene, cam) for name, scene, cam in A.all_scenes()}
SUMS = (("d_mean", "mean"), ("d_conic", "conic"), ("d_cov", "cov"), ("d_op", "op"))      # walk_ref's name, blend_tile_backward's


@functools.lru_cache(maxsize=None)
def state_of(name):
    scene, cam = SCENES[name]
    return cpu_oracle.forward(scene, cam)


@functools.lru_cache(maxsize=None)
def replay_of(name, semantics):
    st, cam = state_of(name), SCENES[name][1]
    return R.replay(st["means2D"], st["conicOpacity"], st["ranges"], st["values"], cam.width, cam.height, R.T_CUTOFF[semantics])


def _close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, what
    assert (np.abs(a - b) <= 1e-12 * np.maximum(np.abs(a), np.abs(b))).all(), (what, float(np.abs(a - b).max()))


def _tiles(name):
    """(tx, ty, ids, the tile's extent in the image) of every tile of a scene's state."""
    st, cam = state_of(name), SCENES[name][1]
    gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
    for ty in range(gy):
        for tx in range(gx):
            a, b = (int(v) for v in st["ranges"][ty * gx + tx])
            ids = st["values"][a:b].astype(np.int64) if b > a else np.zeros(0, np.int64)
            yield tx, ty, ids, (ty * 16, min(cam.height, ty * 16 + 16), tx * 16, min(cam.width, tx * 16 + 16))


@pytest.mark.parametrize("semantics", list(R.T_CUTOFF))
@pytest.mark.parametrize("name", list(SCENES))
def test_the_replay_with_empty_hooks_is_the_oracles_bit_for_bit(name, semantics):
    st, cam = state_of(name), SCENES[name][1]
    exp = st if semantics == "gscuda" else cpu_oracle.blend_cutoff(st, cam, t_cutoff=R.T_CUTOFF[semantics])
    final_t, n_contrib, stopped = replay_of(name, semantics)
    assert final_t.dtype == np.float32 and n_contrib.dtype == np.uint32 and stopped.dtype == bool
    assert np.array_equal(final_t.view(np.uint32), exp["finalT"].view(np.uint32))
    assert np.array_equal(n_contrib, exp["nContrib"])


@pytest.mark.parametrize("semantics", list(R.T_CUTOFF))
def test_a_band_of_tile_rows_is_the_frames_rows_and_zeros_outside(semantics):
    st, cam = state_of("edge"), SCENES["edge"][1]
    assert (cam.width, cam.height) == (40, 24)
    whole = replay_of("edge", semantics)
    band = R.replay(st["means2D"], st["conicOpacity"], st["ranges"], st["values"], 40, 24, R.T_CUTOFF[semantics], tile_rows=(1, 2))
    for got, exp in zip(band, whole):
        assert np.array_equal(got[16:].view(np.uint8), exp[16:].view(np.uint8)) and not got[:16].any()
    assert whole[1][:16].any() and whole[1][16:].any()


def test_the_hooks_see_every_blended_record_once_and_the_tile_ends():
    """start / record / end: per tile one start and one end, and the records a pixel's mask names are the pixel's nContrib-th and
    earlier — the sum of the masks is the number of blended (record, pixel) pairs, which the tile decisions count too."""
    st, cam = state_of("edge"), SCENES["edge"][1]
    seen = {"start": [], "end": [], "pairs": 0}

    def record(regs, g, pos, con, dx, dy, power, alpha, T, upd):
        assert upd.any() and int(st["values"][regs["first"] + pos - 1]) == g and (T[upd] > 0).all() and (alpha[upd] >= np.float32(1 / 255)).all()
        regs["last"][upd] = pos
        seen["pairs"] += int(upd.sum())

    def start(tx, ty):
        seen["start"].append((tx, ty))
        return {"first": int(st["ranges"][ty * 3 + tx][0]), "last": np.zeros(256, np.int64)}

    def end(regs, px, py, inside, T, last, done):
        seen["end"].append((int(px[0]) // 16, int(py[0]) // 16))
        assert np.array_equal(regs["last"][inside], last[inside]) and not last[~inside].any()

    R.replay(st["means2D"], st["conicOpacity"], st["ranges"], st["values"], 40, 24, start=start, record=record, end=end)
    assert seen["start"] == seen["end"] == [(tx, ty) for ty in range(2) for tx in range(3)]
    pairs = sum(int(R.tile_decisions(st["means2D"][ids], st["conicOpacity"][ids], tx, ty, 40, 24).pixels.sum())
                for tx, ty, ids, _ in _tiles("edge") if len(ids))
    assert seen["pairs"] == pairs > 1000


@pytest.mark.parametrize("semantics", list(R.T_CUTOFF))
@pytest.mark.parametrize("name", list(SCENES))
def test_the_tile_decisions_scattered_are_the_replays(name, semantics):
    st, cam = state_of(name), SCENES[name][1]
    final_t, n_contrib, _ = replay_of(name, semantics)
    got_t, got_n = np.full((cam.height, cam.width), np.nan), np.full((cam.height, cam.width), -1, np.int64)
    for tx, ty, ids, (ya, yb, xa, xb) in _tiles(name):
        d = R.tile_decisions(st["means2D"][ids], st["conicOpacity"][ids], tx, ty, cam.width, cam.height, R.T_CUTOFF[semantics])
        maps = R.tile_maps(d)
        got_t[ya:yb, xa:xb] = maps["final_t"][: yb - ya, : xb - xa]
        got_n[ya:yb, xa:xb] = maps["n_contrib"][: yb - ya, : xb - xa]
    assert np.array_equal(got_t.astype(np.float32).view(np.uint32), final_t.view(np.uint32))
    assert np.array_equal(got_n, n_contrib)


def _colour_term(d, col, bg, gp):
    """dL_dalpha and its absolute counterpart of a colour term, as oracle/backward_np.blend_tile_backward writes them."""
    cg, cga, ag = col @ gp, np.abs(col) @ np.abs(gp), np.abs(gp)
    wc = d.w * cg
    behind = (d.final_t * (bg @ gp))[None, :] + (wc.sum(axis=0)[None, :] - np.cumsum(wc, axis=0))
    behind_a = (d.final_t * (np.abs(bg) @ ag))[None, :] + ((d.w * cga).sum(axis=0)[None, :] - np.cumsum(d.w * cga, axis=0))
    dL_dalpha = np.where(d.contrib, d.t_before * cg - behind / (1.0 - np.where(d.contrib, d.alpha, 0.0)), 0.0)
    return dL_dalpha, np.where(d.free, d.t_before * cga + behind_a / (1.0 - np.where(d.free, d.alpha, 0.0)), 0.0)


@pytest.mark.parametrize("name", ["edge", "clamp"])
def test_the_geometry_sums_and_scales_are_the_oracles(name):
    st, cam = state_of(name), SCENES[name][1]
    gc, _, _ = A.pixel_gradients(cam)
    bg = np.asarray(A.BACKGROUND, np.float64)
    seen = partly = 0
    for tx, ty, ids, (ya, yb, xa, xb) in _tiles(name):
        tile_g = np.zeros((3, 16, 16))
        tile_g[:, : yb - ya, : xb - xa] = gc[:, ya:yb, xa:xb]
        xy, co, col = st["means2D"][ids], st["conicOpacity"][ids], st["rgb"][ids]
        exp = B.blend_tile_backward(xy, co, col, tx, ty, cam.width, cam.height, bg, tile_g, f32_forward=True, magnitudes=True)
        d = R.tile_decisions(xy, co, tx, ty, cam.width, cam.height)
        assert d.L == len(ids) > 0
        gp = tile_g.reshape(3, -1) * d.inside[None, :]
        got = R.geometry_sums(d, *_colour_term(d, col.astype(np.float64), bg, gp), shares=True)
        for mine, theirs in SUMS:
            _close(got[mine], exp["d_" + theirs].reshape(got[mine].shape), (name, tx, ty, mine))
            _close(got["M_" + mine], exp["M_" + theirs].reshape(got[mine].shape), (name, tx, ty, "M_" + mine))
        assert (np.abs(got["d_mean"]) <= got["A_d_mean"] * (1 + 1e-12)).all() and (got["A_d_mean"] <= got["M_d_mean"] * (1 + 1e-12)).all()
        assert np.array_equal(d.k, exp["k"]) and np.array_equal(d.pixels, exp["pixels"]) and np.array_equal(d.free_pixels, exp["free_pixels"])
        assert np.array_equal(d.blended, d.contrib.sum(axis=0)) and np.array_equal(d.pixels, d.contrib.sum(axis=1))
        maps = R.tile_maps(d)
        assert np.array_equal(maps["n_contrib"], exp["n_contrib"]) and np.array_equal(maps["final_t"], exp["final_t"])
        seen += int(d.pixels.sum())
        partly += int(((d.free_pixels > 0) & (d.free_pixels < d.pixels)).sum())
    assert seen > 0
    if name == "clamp":
        assert partly >= 12, partly           # records clamped on some of the pixels that blend them and free on the others


def test_float64_forward_is_the_oracles_too():
    """f32_forward=False: the forward finite differences are taken of, blend_tile_backward's default."""
    st, cam = state_of("edge"), SCENES["edge"][1]
    tx, ty, ids, _ = next(t for t in _tiles("edge") if len(t[2]) > 20)
    xy, co, col = st["means2D"][ids], st["conicOpacity"][ids], st["rgb"][ids]
    tile_g = np.random.default_rng(7).normal(size=(3, 16, 16))
    bg = np.asarray(A.BACKGROUND, np.float64)
    exp = B.blend_tile_backward(xy, co, col, tx, ty, 40, 24, bg, tile_g, magnitudes=True)
    d = R.tile_decisions(xy, co, tx, ty, 40, 24, f32_forward=False)
    got = R.geometry_sums(d, *_colour_term(d, col.astype(np.float64), bg, tile_g.reshape(3, -1) * d.inside[None, :]))
    for mine, theirs in SUMS:
        _close(got[mine], exp["d_" + theirs].reshape(got[mine].shape), mine)
        _close(got["M_" + mine], exp["M_" + theirs].reshape(got[mine].shape), "M_" + mine)
    assert np.array_equal(R.tile_maps(d)["final_t"], exp["final_t"]) and np.array_equal(d.k, exp["k"])


SHAPES = {"d_mean": (0, 2), "d_conic": (0, 3), "d_op": (0, 1), "d_cov": (0, 3), "d_chan": (0, 5)}


def test_an_empty_list_and_a_tile_outside_the_image_give_zeros_of_the_right_shapes():
    sums = R.with_scales(R.GEOMETRY + (("d_chan", 5),))
    assert [n for n, _ in sums] == list(SHAPES) + ["M_" + n for n in SHAPES]
    # L == 0, on a partial tile of a 40 x 24 image
    d = R.tile_decisions(np.zeros((0, 2)), np.zeros((0, 4)), 2, 1, 40, 24)
    res = R.empty_tile(d, sums, "k", out=np.zeros((16, 16)))
    assert d.L == 0 and int(d.inside.sum()) == 8 * 8
    for name, shape in SHAPES.items():
        for key in (name, "M_" + name):
            assert res[key].shape == shape and res[key].dtype == np.float64
    for key in ("k", "pixels", "free_pixels"):
        assert res[key].shape == (0,) and res[key].dtype == np.int64
    assert res["n_contrib"].shape == (16, 16) and res["n_contrib"].dtype == np.int64 and not res["n_contrib"].any()
    assert np.array_equal(res["final_t"], d.inside.reshape(16, 16).astype(np.float64)) and res["out"].shape == (16, 16)
    assert set(res) == {n for n, _ in sums} | {"k", "pixels", "free_pixels", "final_t", "n_contrib", "out"}
    # every pixel of the tile outside the image: nothing is blended, whatever the list holds
    st = state_of("edge")
    ids = st["values"][:40].astype(np.int64)
    d = R.tile_decisions(st["means2D"][ids], st["conicOpacity"][ids], 3, 0, 40, 24)
    assert d.L == 40 and not d.inside.any() and not d.contrib.any()
    got = R.geometry_sums(d, np.ones((40, 256)), np.zeros((40, 256)), shares=True)
    for name, (_, width) in list(SHAPES.items())[:4]:
        for key in (name, "M_" + name):
            assert got[key].shape == (40, width) and not got[key].any()
    assert got["A_d_mean"].shape == (40, 2) and not got["A_d_mean"].any()
    maps = R.tile_maps(d)
    assert not d.k.any() and not maps["pixels"].any() and not maps["free_pixels"].any() and maps["pixels"].shape == (40,)
    assert not maps["final_t"].any() and not maps["n_contrib"].any() and maps["final_t"].shape == (16, 16)
