"""GPU: the render backward's block-list feed (csrc/backward.hip: render_backward_kernel's block iterator, block_acc_fits,
zero_block_acc_kernel / flush_block_acc_kernel) Gaussian by Gaussian on frames of several blocks.

tests/test_gpu_backward_edges.py compares every Gaussian with the float64 oracle on its own scale, but on frames of one block;
the frames of several blocks elsewhere are held to whole-frame tolerances. Here the per-Gaussian oracle and bound of
helpers.py (oracle_gradients, assert_backward_inputs, assert_backward_per_gaussian, BW_TAU / BW_C) meet the frames the block
feed was written for. The scenes (helpers.block_scene_a / block_scene_c; tuned and their preconditions shown without a GPU in
tests/test_backward_block_scenes_cpu.py):

  A   272 x 144: 17 x 9 tiles, 3 x 2 blocks, the last block column one tile wide and the last block row one tile high.
      Block (0,0) holds more than two units (2 x 2048 entries) of tiny faint splats and its deepest last contributor lies
      in the third unit; block (1,0) holds between one and two units with the deepest last contributor in the second, and
      opaque stacks that end pixels early; the four edge blocks hold a few hundred ordinary splats and stacks; splats on
      the block corners are entries of two and four blocks, and the frame-wide faint splats entries of all six.
      A12: 6.0 <= R / E_total < 6.5 — twelve floats per entry fit into the 2 R floats of scratch, thirteen do not.
      A13: R / E_total >= 6.6 — thirteen fit as well.
  C   128 x 128, one block of more than 64 units (133 000 tiny splats), direct atomics from the block lists.

Which way every block takes — per-entry float sums or direct atomics — is derived on the host from the forward state
(helpers.block_feed_facts, which says how, and that the derivation of the entries was read off csrc/blockbin.hip) and asserted:
a change of the rule fails these tests instead of emptying them. What no per-Gaussian test reached before, and which case
hits it by an asserted condition:

  1. block index with nbx > 1, partial blocks at the right and bottom edge     every A case: ways asserted for all six blocks
  2. the global entry index as the per-entry key in blocks other than block 0;  A12 / A13 "block lists": blocks (1,0) .. (2,1)
     a Gaussian that is an entry of several blocks, flushed once per block       per-entry; blindness guard (a)
  3. per-entry and direct blocks in one launch, also with the sorted lists      A12 / A13 "block lists" (deep block direct from
     written (sorted = point_list && !per_entry, per tile)                       the block lists), "beside sorted lists" (from
                                                                                 the sorted list)
  4. a per-entry block that crosses the unit boundary (walked == 2) beside a    A12 / A13: p_b >= 2048 in (1,0), p_b >= 4096 in
     block with walked >= 3                                                      (0,0); guard (c)
  5. walked_slice on walked lengths that are no multiple of 4 or 16             asserted on the per-entry blocks' E_b
  6. blocks outside / half inside a band of tile rows, with the block feed      "band through a block": rows 3 .. 8
  7. the thirteenth per-entry float (kAcc = 13); twelve fit, thirteen do not    depth on A13 (blocks per-entry), on A12 (every
                                                                                 block direct while the same frame without
                                                                                 depth is per-entry)
  8. the `below` loop of render_backward_kernel past 64 units                   C: E_b > 64 x 2048 and p_b >= 64 x 2048; guard

The band's reference is the whole frame's, restricted to the band's tiles (helpers.restricted_reference): a band call bins
only its rows, and the lists of its tiles are those of the full frame — its forward state is compared with that reference
bit for bit before its backward, as every variant's is. The blindness guards (a block's share, the edge blocks' tiles, the
records past a unit boundary lost: each leaves the bound by a factor of ten on many Gaussians) are asserted here on the GPU's
forward state as they are on the CPU's.
"""
import numpy as np
import pytest

import helpers as Hh
from helpers import assert_backward_inputs, assert_backward_per_gaussian, gradients_of, oracle_gradients

pytestmark = pytest.mark.gpu

BG = (0.3, 0.1, 0.6)
BAND = (3, 9)
THREADS = 8
WAYS_MIXED = {(0, 0): "direct", (1, 0): "per_entry", (2, 0): "per_entry", (0, 1): "per_entry", (1, 1): "per_entry", (2, 1): "per_entry"}
_cache = {}


def _frame(name, semantics="gscuda"):
    """One rasterizer, forward-state snapshot and float64 reference per scene and profile, computed once and left unchanged."""
    key = (name, semantics)
    if key in _cache:
        return _cache[key]
    import torch
    from gsrast_amd.rasterizer import SplatRasterizer
    scene, cam = Hh.block_scene_c() if name == "C" else Hh.block_scene_a(Hh.BLOCK_SCENE_A_FILL[name])
    w, h = cam.width, cam.height
    gx, gy = (w + 15) // 16, (h + 15) // 16
    kw = dict(semantics=semantics, sh_degree=0)
    cutoff = 1e-4 if semantics == "inria" else 1e-3
    r = SplatRasterizer(w, h, background=BG)
    r.configure_from_scene(scene)
    dL, gd = Hh.block_scene_gradient(w, h)
    r.draw(cam, plan="sort", tile_history=False, **kw)
    assert r.last_num_rendered > 0 and r.last_lists_written
    snap = Hh.host_snapshot(r)
    f = dict(name=name, r=r, scene=scene, cam=cam, kw=kw, cutoff=cutoff, snap=snap, dL_host=dL, gd_host=gd,
             dL=torch.from_numpy(dL).cuda(), gd=torch.from_numpy(gd).cuda(), depth_refs={})
    if name == "C":
        f["tiles"] = list(Hh.BLOCK_SCENE_C_TILES)
        f["targets"] = Hh.scene_c_targets(snap, f["tiles"])
        f["groups"] = Hh.block_group_of_tile(w, h)
    else:
        f["tiles"] = [(tx, ty) for ty in range(gy) for tx in range(gx)]
        f["targets"] = np.arange(r.num_gaussians)
        f["groups"] = Hh.block_group_of_tile(w, h, BAND[0])
    f["ref"] = oracle_gradients(snap, dL, BG, f["tiles"], f["targets"], 4096, f32_forward=True, magnitudes=True, t_cutoff=cutoff,
                                full_lists=True, group_of_tile=f["groups"], threads=THREADS)
    assert_backward_inputs(snap.state["nContrib"], snap.state["finalT"], f["ref"], f"{name}, sorted lists")
    f["facts"] = {False: Hh.block_feed_facts(snap), True: Hh.block_feed_facts(snap, depth=True)}
    assert f["facts"][False]["R"] == r.last_num_rendered
    print(f"[blocks] {name} ({semantics}): N={r.num_gaussians}, {Hh.describe_block_ways(f['facts'][False])}")
    if name != "C":
        nb = f["facts"][False]["nbx"] * f["facts"][False]["nby"]
        f["ref_band"] = Hh.restricted_reference(f["ref"], [2 * b + 1 for b in range(nb)], w, h)
        f["facts_band"] = Hh.block_feed_facts(snap, rows=BAND)
    _cache[key] = f
    return f


def _depth_ref(f, mode):
    """The reference of a backward with the depth channel: the colour pass plus the pass of colours (d_i, 0, 0)."""
    if mode not in f["depth_refs"]:
        from test_depth_cpu import depth_values_f32
        d = depth_values_f32(f["scene"]["means3D"], np.asarray(f["cam"].view, np.float32), mode == "inverse").astype(np.float64)
        g3 = np.zeros_like(f["dL_host"])
        g3[0] = f["gd_host"]
        ref_d = oracle_gradients(f["snap"], g3, BG, f["tiles"], f["targets"], 4096, f32_forward=True, magnitudes=True,
                                 t_cutoff=f["cutoff"], full_lists=True, colors=np.stack([d, 0 * d, 0 * d], 1), background=(0.0, 0.0, 0.0),
                                 threads=THREADS)
        f["depth_refs"][mode] = Hh.depth_superposition(f["ref"], ref_d)
    return f["depth_refs"][mode]


def _assert_scene_a_ways(f, name, depth):
    """The required facts of scene A (the issue's table), on the GPU's own forward state."""
    facts = f["facts"][depth]
    ratio = facts["R"] / facts["E_total"]
    if name == "A12":
        assert 6.0 <= ratio < 6.5, ratio
        Hh.assert_block_ways(facts, "direct" if depth else WAYS_MIXED, f"{name}, depth {depth}")
    else:
        assert ratio >= 6.6, ratio
        Hh.assert_block_ways(facts, WAYS_MIXED, f"{name}, depth {depth}")
    b = facts["blocks"]
    assert (facts["nbx"], facts["nby"]) == (3, 2) and len(b[(2, 0)]["tiles"]) == 8 and len(b[(0, 1)]["tiles"]) == 8 and len(b[(2, 1)]["tiles"]) == 1
    assert b[(0, 0)]["p"] >= 2 * Hh.K_UNIT and Hh.K_UNIT <= b[(1, 0)]["p"] and b[(1, 0)]["E"] <= 2 * Hh.K_UNIT
    per_entry = [k for k, v in b.items() if v["way"] == "per_entry"]
    if per_entry:
        assert any(b[k]["E"] % 4 != 0 for k in per_entry) and any(b[k]["E"] % 16 not in (0, 4, 8, 12) for k in per_entry)
        for k in per_entry:          # pixels ended early by the transmittance cut-off in every per-entry block
            assert sum(int((f["ref"]["stop_idx"][ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] >= 0).sum()) for tx, ty in b[k]["tiles"]) >= 20, k
    assert sum(len(keys) >= 2 for keys in facts["membership"].values()) >= 100
    return facts


def _draw_block_fed(f, lists, rows=None):
    r = f["r"]
    dkw = dict(plan="blocks", overlap_emit=True) if lists else dict(plan="blocks", sorted_lists=False)
    r.draw(f["cam"], tile_rows=rows, tile_history=False, **dkw, **f["kw"])
    assert r.last_plan == "blocks" and not r.last_blend_from_lists, (r.last_plan, r.last_blend_from_lists)
    assert r.last_lists_written == lists
    return r


def _check(f, got, ref, facts, wide, what):
    floats = np.ones(len(f["targets"]), bool) if not wide else Hh.float_sum_gaussians(facts, f["targets"])
    return assert_backward_per_gaussian(gradients_of(got, f["targets"]), ref, float_tile_sums=floats, what=what), floats


A_VARIANTS = ("block lists", "block lists, float sums", "block lists beside sorted lists", "band through a block", "second call")


@pytest.mark.parametrize("variant", A_VARIANTS)
@pytest.mark.parametrize("name", ["A12", "A13"])
def test_block_feed_per_gaussian_on_several_blocks(name, variant):
    f = _frame(name)
    facts = _assert_scene_a_ways(f, name, depth=False)
    wide = variant != "block lists, float sums"
    band = variant == "band through a block"
    rows = BAND if band else None
    ref = f["ref_band"] if band else f["ref"]
    if band:
        facts = f["facts_band"]
        Hh.assert_block_ways(facts, "per_entry" if name == "A13" else "direct", f"{name}, band")
        # the band cuts through block row 0 (tile rows 3 .. 7 of it) and holds block row 1
        assert [len(v["tiles"]) for v in facts["blocks"].values()] == [40, 40, 5, 8, 8, 1]
    r = _draw_block_fed(f, lists=variant == "block lists beside sorted lists", rows=rows)
    assert r.last_num_rendered == facts["R"], (r.last_num_rendered, facts["R"])
    im = r.map_image_state()
    what = f"{name}, {variant}"
    assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), ref, what)
    for call in range(2 if variant == "second call" else 1):        # (second call: the per-entry words were cleared again)
        got = r.backward(f["dL"], tile_rows=rows, wide_sums=wide, **f["kw"])
        worst, _ = _check(f, got, ref, facts, wide, what + (f", call {call + 1}" if variant == "second call" else ""))
    print(f"[blocks] {what}: worst ratio {worst:.2e}; {Hh.describe_block_ways(facts)}")


def test_block_feed_per_gaussian_upstream_profile():
    """A13 under the upstream profile (cut-off 1e-4, its own pixel centres: its own R, entries and reference)."""
    f = _frame("A13", "inria")
    facts = f["facts"][False]
    Hh.assert_block_ways(facts, WAYS_MIXED, "A13, upstream profile")
    r = _draw_block_fed(f, lists=False)
    im = r.map_image_state()
    assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), f["ref"], "A13, upstream profile")
    got = r.backward(f["dL"], wide_sums=True, **f["kw"])
    _check(f, got, f["ref"], facts, True, "A13, upstream profile, block lists")


@pytest.mark.parametrize("wide", [True, False], ids=["wide sums", "float sums"])
@pytest.mark.parametrize("mode", [True, "inverse"], ids=["depth", "inverse depth"])
@pytest.mark.parametrize("name", ["A12", "A13"])
def test_block_feed_per_gaussian_with_the_depth_channel(name, mode, wide):
    """kAcc = 13: the thirteenth per-entry float (A13), and the frame where twelve fit and thirteen do not (A12: direct atomics
    from the block lists in every block, while the same call without depth takes per-entry sums)."""
    f = _frame(name)
    _assert_scene_a_ways(f, name, depth=False)
    facts = _assert_scene_a_ways(f, name, depth=True)
    ref = _depth_ref(f, mode)
    r = _draw_block_fed(f, lists=False)
    im = r.map_image_state()
    what = f"{name}, block lists, {'inverse ' if mode == 'inverse' else ''}depth, {'wide' if wide else 'float'} sums"
    assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), ref, what)
    got = r.backward(f["dL"], dL_ddepth=f["gd"], depth=mode, wide_sums=wide, **f["kw"])
    _, floats = _check(f, got, ref, facts, wide, what)
    Hh.assert_depth_sums_per_gaussian(got["dL_ddepths"].cpu().numpy()[f["targets"]], ref, float_tile_sums=floats, what=what)


@pytest.mark.parametrize("wide", [True, False], ids=["wide sums", "float sums"])
def test_block_feed_per_gaussian_past_64_units(wide):
    """Scene C: the second iteration of the `below` loop (a block of more than 64 units), on six tiles of the block."""
    f = _frame("C")
    facts = f["facts"][False]
    b = facts["blocks"][(0, 0)]
    assert len(facts["blocks"]) == 1 and b["E"] > 64 * Hh.K_UNIT and b["p"] >= 64 * Hh.K_UNIT, Hh.describe_block_ways(facts)
    Hh.assert_block_ways(facts, "direct", "C")
    assert len(f["targets"]) >= 1000
    r = _draw_block_fed(f, lists=False)
    im = r.map_image_state()
    what = f"C, block lists, {'wide' if wide else 'float'} sums"
    assert_backward_inputs(im["nContrib"].cpu().numpy(), im["finalT"].cpu().numpy(), f["ref"], what)
    got = r.backward(f["dL"], wide_sums=wide, **f["kw"])
    _check(f, got, f["ref"], facts, wide, what)
    invisible = np.nonzero(f["snap"].state["tilesTouched"] == 0)[0]
    assert len(invisible) >= 100
    for k, v in got.items():
        assert not v.cpu().numpy()[invisible].any(), (what, k, "a Gaussian without a tile must get exactly zero")


def test_blindness_guards_on_the_gpu_state():
    """The bound sees the loss of a block's share (a), of the edge blocks' tiles (b), of the records past a unit boundary
    (c; C: past 64 units): each faulted reference leaves it by a factor of ten on many Gaussians."""
    f = _frame("A13")
    g = Hh.block_blindness_guards_a(f["ref"], f["facts"][False], f["targets"])
    print(f"[blocks] A13 guards: {g}")
    seen, of = g["a"]
    assert of >= 100 and 2 * seen >= of and g["b"] >= 20 and g["c"] >= 20, g
    c = _frame("C")
    seen_c = Hh.block_blindness_guard_c(c["ref"], c["facts"][False], c["targets"])
    print(f"[blocks] C guard: {seen_c}")
    assert seen_c >= 20
