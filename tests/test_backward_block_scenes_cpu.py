"""CPU: the scenes of tests/test_gpu_backward_blocks.py hit what they are meant to hit, shown on the C++ oracle's forward state
(oracle/cpu_oracle.forward: the state the GPU reproduces bit for bit, which the GPU tests re-check with assert_backward_inputs)
and the float64 backward oracle — this is where the scenes are tuned, without a GPU.

Per scene: the window of R / E_total, every block's E_b and p_b and with them the way its per-Gaussian sums take in gsr_backward
(helpers.block_feed_facts: the one copy of that derivation), pixels that end early in per-entry blocks, the longest tile list,
and the blindness guards: the per-Gaussian bound of helpers.assert_backward_per_gaussian sees, by a factor of ten, the loss of a
block's share, of the edge blocks' tiles, and of the records past a unit boundary.
"""
import numpy as np
import pytest

import helpers as Hh

BG = (0.3, 0.1, 0.6)
_cache = {}


def _scene_a(name):
    """(HostForwardState, reference over the whole frame with per-block groups, camera) of scene A12 / A13, computed once."""
    if name not in _cache:
        from oracle import cpu_oracle
        scene, cam = Hh.block_scene_a(Hh.BLOCK_SCENE_A_FILL[name])
        r = Hh.HostForwardState(cpu_oracle.forward(scene, cam, background=BG, threads=4), cam)
        w, h = cam.width, cam.height
        dL, _ = Hh.block_scene_gradient(w, h)
        tiles = [(tx, ty) for ty in range((h + 15) // 16) for tx in range((w + 15) // 16)]
        ref = Hh.oracle_gradients(r, dL, BG, tiles, np.arange(r.num_gaussians), 4096, f32_forward=True, magnitudes=True,
                                  full_lists=True, group_of_tile=Hh.block_group_of_tile(w, h, 3), threads=4)
        # (the float32 forward of the backward oracle is the C++ oracle's, bit for bit: the contract the GPU tests rest on)
        Hh.assert_backward_inputs(r.state["nContrib"], r.state["finalT"], ref, name)
        _cache[name] = (r, ref, cam)
    return _cache[name]


WAYS_MIXED = {(0, 0): "direct", (1, 0): "per_entry", (2, 0): "per_entry", (0, 1): "per_entry", (1, 1): "per_entry", (2, 1): "per_entry"}


def test_pixel_splats_is_the_edges_files_placement():
    """The vectorised placement against the per-row one of tests/test_gpu_backward_edges.py, row by row."""
    import test_gpu_backward_edges as E
    cam = Hh.block_scene_camera(272, 144)
    rows = Hh._rows(np.random.default_rng(3), 40, (-20, 290), (-20, 160), (-2.0, 1.5), (0.0, 60.0), (0.01, 1.0))
    a = E._splats(cam, [(r[0], r[1], r[2], r[3], r[4], r[5:8]) for r in rows])
    b = Hh.pixel_splats(cam, rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4], rows[:, 5:8])
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, k
        assert np.allclose(a[k], b[k], rtol=1e-6, atol=1e-6), k


@pytest.mark.parametrize("name", ["A12", "A13"])
def test_scene_a_hits_its_block_ways(name):
    r, ref, cam = _scene_a(name)
    w, h = cam.width, cam.height
    gx, gy = (w + 15) // 16, (h + 15) // 16
    assert (gx, gy) == (17, 9)                      # 3 x 2 blocks, the last column one tile wide, the last row one tile high
    plain, deep = Hh.block_feed_facts(r), Hh.block_feed_facts(r, depth=True)
    print(f"[block scenes] {name}: {Hh.describe_block_ways(plain)}")
    assert (plain["nbx"], plain["nby"]) == (3, 2) and plain["R"] == r.last_num_rendered
    ratio = plain["R"] / plain["E_total"]
    assert plain["E_total"] <= plain["R"]           # (the entries' indices live in the R words of valuesUnsorted)
    lengths = np.diff(r.state["ranges"].astype(np.int64), axis=1)
    assert lengths.max() <= 4096, lengths.max()     # the oracle's max_depth
    if name == "A12":
        assert 6.0 <= ratio < 6.5, ratio            # twelve floats per entry fit, thirteen do not
        Hh.assert_block_ways(plain, WAYS_MIXED, name)
        Hh.assert_block_ways(deep, "direct", name + ", depth")
        assert plain["fits"] and not deep["fits"]
    else:
        assert ratio >= 6.6, ratio
        Hh.assert_block_ways(plain, WAYS_MIXED, name)
        Hh.assert_block_ways(deep, WAYS_MIXED, name + ", depth")
    b = plain["blocks"]
    assert b[(0, 0)]["E"] > 2 * Hh.K_UNIT and b[(0, 0)]["p"] >= 2 * Hh.K_UNIT           # the blend looked into three units
    assert b[(1, 0)]["E"] <= 2 * Hh.K_UNIT and b[(1, 0)]["p"] >= Hh.K_UNIT             # ... and here into exactly two
    # the global entry index of a block other than block 0 starts past block 0's entries; Gaussians that are entries of several blocks
    multi = [g for g, keys in plain["membership"].items() if len(keys) >= 2]
    assert len(multi) >= 100 and max(len(keys) for keys in plain["membership"].values()) == 6
    # walked_slice: lengths that are no multiple of 4 (and so of 16) among the per-entry blocks (the walked part of a block of
    # one unit, and of the two-unit block whose last unit the blend looked into, is its whole list)
    per_entry = [k for k, v in b.items() if v["way"] == "per_entry"]
    assert any(b[k]["E"] % 4 != 0 for k in per_entry) and any(b[k]["E"] % 16 not in (0, 4, 8, 12) for k in per_entry)
    # pixels that end early (the transmittance cut-off) in every per-entry block; none in the deep block
    for k in per_entry:
        ended = sum(int((ref["stop_idx"][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] >= 0).sum()) for tx, ty in b[k]["tiles"])
        assert ended >= 20, (k, ended)
        short = sum(int((r.state["nContrib"][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] < lengths[ty * gx + tx]).sum()) for tx, ty in b[k]["tiles"])
        assert short >= ended
    # the band of tile rows 3 .. 8: rows 3 .. 7 of block row 0, and block row 1; its ways from its own R and entries
    band = Hh.block_feed_facts(r, rows=(3, 9))
    print(f"[block scenes] {name}, band: {Hh.describe_block_ways(band)}")
    Hh.assert_block_ways(band, "per_entry" if name == "A13" else "direct", name + ", band")
    assert band["R"] < plain["R"] and all(len(v["tiles"]) in (40, 8, 5, 1) for v in band["blocks"].values())
    ref_band = Hh.restricted_reference(ref, [2 * i + 1 for i in range(6)], w, h)
    assert int((ref_band["pixels"] > 0).sum()) >= 1000 and (ref_band["n_contrib"][:48] == -1).all() and (ref_band["n_contrib"][48:] >= 0).all()


def test_scene_a13_upstream_profile_block_ways():
    """The upstream profile's frame of A13 (another pixel-centre convention: other rectangles, another R and E)."""
    from oracle import inria_np
    scene, cam = Hh.block_scene_a(Hh.BLOCK_SCENE_A_FILL["A13"])
    r = Hh.HostForwardState(inria_np.forward(scene, cam, BG, deg=0, blend_with="cpp", threads=4), cam)
    facts = Hh.block_feed_facts(r)
    print(f"[block scenes] A13, upstream profile: {Hh.describe_block_ways(facts)}")
    Hh.assert_block_ways(facts, WAYS_MIXED, "A13, upstream profile")


def test_scene_a13_blindness_guards():
    r, ref, cam = _scene_a("A13")
    facts = Hh.block_feed_facts(r)
    g = Hh.block_blindness_guards_a(ref, facts, np.arange(r.num_gaussians))
    print(f"[block scenes] A13 guards: {g}")
    seen, of = g["a"]
    assert of >= 100 and 2 * seen >= of, g          # (a) a block's share lost
    assert g["b"] >= 20, g                          # (b) the tiles of block column 2 and block row 1 lost
    assert g["c"] >= 20, g                          # (c) block (1,0)'s records from position 2048 on lost


def test_scene_c_has_more_than_64_units_and_its_guard():
    from oracle import cpu_oracle
    scene, cam = Hh.block_scene_c()
    r = Hh.HostForwardState(cpu_oracle.forward(scene, cam, background=BG, threads=4), cam)
    facts = Hh.block_feed_facts(r)
    print(f"[block scenes] C: {Hh.describe_block_ways(facts)}")
    b = facts["blocks"][(0, 0)]
    assert len(facts["blocks"]) == 1 and b["E"] > 64 * Hh.K_UNIT and b["p"] >= 64 * Hh.K_UNIT
    Hh.assert_block_ways(facts, "direct", "C")
    assert not facts["fits"] and facts["E_total"] <= facts["R"]
    lengths = np.diff(r.state["ranges"].astype(np.int64), axis=1)
    assert 2048 < lengths.min() and lengths.max() <= 4096, (lengths.min(), lengths.max())
    assert int((r.state["tilesTouched"] == 0).sum()) >= 100          # Gaussians without a tile: their gradients stay zero
    targets = Hh.scene_c_targets(r, Hh.BLOCK_SCENE_C_TILES)
    dL, _ = Hh.block_scene_gradient(cam.width, cam.height)
    ref = Hh.oracle_gradients(r, dL, BG, list(Hh.BLOCK_SCENE_C_TILES), targets, 4096, f32_forward=True, magnitudes=True,
                              full_lists=True, group_of_tile=Hh.block_group_of_tile(cam.width, cam.height), threads=4)
    Hh.assert_backward_inputs(r.state["nContrib"], r.state["finalT"], ref, "C")
    seen = Hh.block_blindness_guard_c(ref, facts, targets)
    print(f"[block scenes] C: {len(targets)} targets, guard {seen}")
    assert len(targets) >= 1000 and seen >= 20, (len(targets), seen)
