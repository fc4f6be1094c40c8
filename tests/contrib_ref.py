"""Reference of the per-Gaussian contribution statistics (include/gsrast_amd_contrib.h): the float32 replay of the
blend loop that tests/walk_ref.py holds (the masks, the operation order, exp = the C++ oracle's libm expf) over given arrays,
with hooks that keep q = (uint32)(alpha T 2^32) of every blended (record, pixel) instead of a colour. Shared by
tests/test_contrib_cpu.py and tests/test_gpu_contrib.py; also the scenes both files use, so that what the CPU file establishes
of a scene (the replay's finalT / nContrib are cpu_oracle.forward's bit for bit; the blindness guards) holds for the arrays
the GPU file compares."""
import functools
import types

import numpy as np

import walk_ref
from walk_ref import T_CUTOFF

F = np.float32
NAMES = ("weight_sum", "weight_max", "pixels", "dominant")
DTYPES = {"weight_sum": np.uint64, "weight_max": np.uint32, "pixels": np.uint64, "dominant": np.uint64}


def contribution(means2D, conic_opacity, ranges, values, W, H, t_cutoff=0.001, tile_rows=None, exp=None, wide=False):
    """The four integer arrays [N] over the tiles of rows `tile_rows` (default: all), and finalT / nContrib [H, W] of the
    replay (zeros outside those rows). wide: alpha, T and w in float64 instead (the decisions stay the float32 replay's: both
    run side by side), and no fixed point — returns {"weight_sum_f64": float64[N]} beside the rest."""
    n = np.asarray(means2D).size // 2
    out = {k: np.zeros(n, DTYPES[k]) for k in NAMES}
    wide_sum = np.zeros(n, np.float64)
    scale = F(4294967296.0)

    def start(tx, ty):
        return types.SimpleNamespace(T64=np.ones(256, np.float64), best=np.zeros(256, np.uint32), best_id=np.full(256, -1, np.int64))

    def record(r, g, pos, con, dx, dy, power, alpha, T, upd):
        w = (alpha * T).astype(F)
        q = np.trunc((w * scale).astype(F).astype(np.float64)).astype(np.uint64)[upd]       # (the product by 2^32 is exact)
        assert (q > 0).all() and (q < (1 << 32)).all()
        out["weight_sum"][g] += np.uint64(int(q.sum()))
        out["weight_max"][g] = max(int(out["weight_max"][g]), int(q.max()))
        out["pixels"][g] += np.uint64(int(upd.sum()))
        better = np.zeros(256, bool)
        better[upd] = q.astype(np.uint32) > r.best[upd]               # strict: a tie stays with the front-most
        r.best[better] = q.astype(np.uint32)[better[upd]]
        r.best_id[better] = g
        if wide:
            d = (dx.astype(np.float64), dy.astype(np.float64))
            p64 = -0.5 * (float(con[0]) * d[0] * d[0] + float(con[2]) * d[1] * d[1]) - float(con[1]) * d[0] * d[1]
            a64 = np.minimum(float(F(0.99)), float(con[3]) * np.exp(p64))
            wide_sum[g] += float((a64 * r.T64)[upd].sum())
            r.T64[upd] = (r.T64 * (1.0 - a64))[upd]

    def end(r, px, py, inside, T, last, done):
        np.add.at(out["dominant"], r.best_id[inside & (r.best > 0)], np.uint64(1))

    finalT, ncontrib, stopped = walk_ref.replay(means2D, conic_opacity, ranges, values, W, H, t_cutoff, tile_rows, exp, start, record, end)
    out.update(finalT=finalT, nContrib=ncontrib, stopped=stopped)          # (stopped: the pixel ended on the cut-off)
    if wide:
        out["weight_sum_f64"] = wide_sum
    return out


def of_state(state, cam, semantics="gscuda", tile_rows=None, **kw):
    """contribution() over a forward state (cpu_oracle.forward's dict, or the arrays read back from the GPU under those names)."""
    return contribution(state["means2D"], state["conicOpacity"], state["ranges"], state["values"], cam.width, cam.height,
                        T_CUTOFF[semantics], tile_rows, **kw)


def add(a, b):
    """What two calls into the same arrays leave: sums add, maxima take the larger."""
    return {k: (np.maximum(a[k], b[k]) if k == "weight_max" else a[k] + b[k]) for k in NAMES}


# ---- scenes ---------------------------------------------------------------------------------------------------------------
LIST_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 600)       # the wave's batch of 64 and the reference's round of 256


def _camera(w, h):
    from helpers import block_scene_camera
    return block_scene_camera(w, h)


def _splats(cam, rows):
    from helpers import pixel_splats
    rows = np.asarray(rows, np.float64)
    return pixel_splats(cam, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:8])


def _rows(rng, n, x, y, z, sig, op):
    from helpers import _rows as rows
    return rows(rng, n, x, y, z, sig, op)


@functools.lru_cache(maxsize=None)
def one_tile_scene(length, opaque):
    """One 16 x 16 tile whose list has exactly `length` records (asserted by the callers from the state). faint: every pixel
    walks to the end of the list. opaque: nearly opaque small splats in front (the first 3/8 of the depth range), so that
    pixels stop at different depths — and some never. Two splats far off the frame have no tile."""
    # (a frame of ONE record leaves its range open, GSCuda.cu:533, and blends nothing: the list of length 1 gets a second tile
    # beside it with a record of its own)
    cam = _camera(32 if length == 1 else 16, 16)
    rng = np.random.default_rng(1000 + length + (7 if opaque else 0))
    rows = _rows(rng, length, (1, 15), (1, 15), (-1.0, 1.0), (0.6, 2.5), (0.004, 0.02) if not opaque else (0.02, 0.3))
    if opaque:
        k = max(1, min(length // 2, 24))
        rows[:k] = _rows(rng, k, (2, 14), (2, 14), (-2.0, -1.2), (1.0, 2.5), (0.9, 0.99))
    else:
        j = np.arange(length) % 5 == 0
        rows[j, 4] = rng.uniform(0.3, 0.6, int(j.sum())) * (0.05 if length > 64 else 1.0) + 0.004     # a few that count, none that saturates
    off = _rows(rng, 2, (-300, -200), (4, 12), (-1.0, 1.0), (0.5, 1.0), (0.5, 0.9))
    if length == 1:
        rows[0, :5] = (6.0, 7.0, 0.0, 1.2, 0.5 if not opaque else 0.999)
        off = np.concatenate([off, _rows(rng, 1, (23, 25), (7, 9), (-1.0, 1.0), (0.6, 0.7), (0.5, 0.9))])
    return _splats(cam, np.concatenate([rows, off])), cam


@functools.lru_cache(maxsize=None)
def edge_scene():
    """40 x 24: partial edge tiles in both directions (3 x 2 tiles), 300 Gaussians of mixed size and opacity, opaque stacks."""
    from helpers import _opaque_stacks
    cam = _camera(40, 24)
    rng = np.random.default_rng(77)
    # (columns 0 and 1 stay out of everybody's reach: pixels that blend nothing; 20 splats stay below 1/255 everywhere)
    rows = np.concatenate([_rows(rng, 250, (8, 42), (-2, 26), (-1.0, 1.0), (0.4, 2.0), (0.004, 0.9)),
                           _rows(rng, 20, (8, 42), (-2, 26), (-1.0, 1.0), (0.4, 2.0), (0.001, 0.0038)),
                           _opaque_stacks(rng, 3, (14, 36), (4, 20)),
                           _rows(rng, 6, (-200, -150), (0, 24), (-1.0, 1.0), (0.5, 1.0), (0.5, 0.9))])
    assert len(rows) == 300
    return _splats(cam, rows), cam


@functools.lru_cache(maxsize=None)
def fill_scene():
    """128 x 128 (8 x 8 tiles): one screen-filling Gaussian in front — 64 tiles add into its row — and 200 small ones."""
    from helpers import _opaque_stacks
    cam = _camera(128, 128)
    rng = np.random.default_rng(78)
    big = np.array([[64.0, 64.0, -1.5, 25.0, 0.35, 0.2, 0.4, 0.6]])      # (alpha >= 1/255 within 75 pixels: every tile, not every pixel)
    rows = np.concatenate([big, _rows(rng, 166, (0, 128), (0, 128), (-1.0, 1.0), (0.5, 5.0), (0.004, 0.9)),
                           _rows(rng, 10, (0, 128), (0, 128), (-1.0, 1.0), (0.5, 5.0), (0.001, 0.0038)),
                           _opaque_stacks(rng, 2, (10, 118), (10, 118)),
                           _rows(rng, 8, (-300, -250), (0, 128), (-1.0, 1.0), (0.5, 1.0), (0.5, 0.9))])
    assert len(rows) == 201
    return _splats(cam, rows), cam


@functools.lru_cache(maxsize=None)
def two_view_scene():
    """The end-to-end scene, seen by two cameras: 48 x 32, sparse and faint enough that no pixel of either view reaches the
    cut-off (asserted by the callers) — removing the Gaussians nothing blended then leaves both pictures as they were, bit for
    bit. Some Gaussians are too faint to pass 1/255 anywhere, some hide in a corner of their tile rectangle."""
    from helpers import posed_camera
    cams = (posed_camera(48, 32, (0.8, 0.4, -5.0), roll=0.3), posed_camera(48, 32, (-0.7, 0.5, -5.2), roll=-0.4))
    rng = np.random.default_rng(79)
    n = 260
    means = np.ones((n, 4), np.float32)
    means[:, 0] = rng.uniform(-2.6, 2.6, n)
    means[:, 1] = rng.uniform(-1.8, 1.8, n)
    means[:, 2] = rng.uniform(-1.0, 1.0, n)
    scales = np.full((n, 4), np.e, np.float32)
    scales[:, :3] = rng.uniform(0.01, 0.12, (n, 3))
    q = rng.normal(size=(n, 4))
    rots = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    op = rng.uniform(0.02, 0.25, n).astype(np.float32)
    op[::4] = rng.uniform(0.001, 0.0038, len(op[::4]))          # below 1/255 everywhere: blended by nobody
    shs = np.zeros((n, 48), np.float32)
    shs[:, :3] = rng.uniform(-1, 1, (n, 3))
    return {"means3D": means, "scales": scales, "rotations": rots, "opacities": op, "shs": shs}, cams


def all_scenes():
    """(name, scene, camera) of every scene the GPU file compares with the reference."""
    for length in LIST_LENGTHS:
        for opaque in (False, True):
            scene, cam = one_tile_scene(length, opaque)
            yield f"tile-{length}-{'opaque' if opaque else 'faint'}", scene, cam
    yield ("edge",) + edge_scene()
    yield ("fill",) + fill_scene()
    scene, cams = two_view_scene()
    for i, cam in enumerate(cams):
        yield f"views-{i}", scene, cam
