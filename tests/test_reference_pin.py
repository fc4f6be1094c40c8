"""CPU: the two oracles (oracle/gsr_oracle.cpp, oracle/oracle_np.py) against the reference ITSELF — its own GSCuda.cu /
AuxBuffer.cu / CudaHelpers.cu compiled for the host against the stand-ins of oracle/ref_host/ (oracle/build_ref.py,
oracle/ref_cpu.py). Every output the reference writes is compared by bytes: both sides are the same float32 operations
under the same compiler flags and the same libm expf, so equality is the requirement, not a tolerance.

What this pins: the reference's text (the `(int) ceil(3.0f * cov.z)` without a square root, the parameter shuffle between
preprocess and preprocessCUDA, `(numGaussians + 255 / 256)` blocks, the tile never closed when R == 1, the doubles of
quatToMat, which overloads of ceil / round / exp are taken). By what: host stand-ins for the CUDA runtime,
cooperative_groups, cub and glm, glm's operation orders restated. What it does NOT pin: float -> int conversions that leave
int or start from NaN (undefined on the host, saturating on the device: test_out_of_range_conversions_...), nvcc's FMA
contraction (tests/test_contraction_sensitivity.py bounds it), CUDA's expf against glibc's, the upstream profile, and the
reference's caller (GSGaussians.cpp) and .ply loader.

The library is built on first use when the reference tree is present; the tests skip only when there is neither a
library nor a tree to build it from.
"""
import ctypes as C
import os

import numpy as np
import pytest

import reference_frames as F
from helpers import ROOT
from oracle import cpu_oracle, oracle_np, points_np, ref_cpu

needs_reference = pytest.mark.skipif(not ref_cpu.available(),
                                     reason="neither oracle/_ref/libgscuda_ref.so nor a reference tree to build it from")
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_frames.npz")


def _bytes_equal(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _differing(ref, got, keys=F.REF_KEYS):
    bad = [k for k in keys if not _bytes_equal(ref[k], got[k])]
    if ref["num_rendered"] != got["num_rendered"]:
        bad.append("num_rendered")
    return bad


def _oracles(scene, cam, bg, kw):
    return (("gsr_oracle.cpp", cpu_oracle.forward(scene, cam, bg, **kw)),
            ("oracle_np.py", oracle_np.forward(scene, cam, bg, exp=cpu_oracle.expf, **kw)))      # (libm's expf, as the other two)


def _pin(frame, what, min_rendered=1):
    """The frame through the reference and both oracles: every output byte for byte. Returns the reference's outputs."""
    scene, cam, bg, kw = frame
    ref = ref_cpu.forward(scene, cam, bg, **kw)
    assert ref["num_rendered"] >= min_rendered, (what, "the reference renders", ref["num_rendered"])
    in_range = F.conversions_in_range(ref, cam)
    assert in_range.all(), (what, "a conversion left int: not a frame a host build pins", np.nonzero(~in_range)[0][:8])
    for name, got in _oracles(scene, cam, bg, kw):
        bad = _differing(ref, got)
        assert not bad, f"{what}: {name} differs from the reference in {bad}"
    print(f"[reference pin] {what}: {cam.width}x{cam.height} N={scene['means3D'].shape[0]} R={ref['num_rendered']}: "
          f"{len(F.REF_KEYS)} outputs byte-equal in both oracles")
    return ref


# ---------------------------------------------------------------- whole frames
@needs_reference
@pytest.mark.parametrize("use_rects", [True, False])
def test_golden_config1_on_both_rectangle_paths(use_rects):
    ref = _pin(F.golden(use_rects), f"config 1, use_rects={use_rects}")
    assert (ref["rects"] is not None) == use_rects


@needs_reference
@pytest.mark.parametrize("seed", range(12))
def test_random_small_frames(seed):
    """The recipes of test_gpu_parity.test_random_small_frames_against_oracle: single tile rows (seed % 4 == 0), single tile
    columns (seed % 4 == 1), partial tiles. Every seed renders something in the reference (asserted, not skipped)."""
    frame = F.random_small_frame(seed)
    cam = frame[1]
    if seed % 4 == 0:
        assert cam.height <= 16
    if seed % 4 == 1:
        assert cam.width <= 16
    _pin(frame, f"random small frame {seed}")


@needs_reference
@pytest.mark.parametrize("w,h,n,seed", F.ANISOTROPIC)
def test_anisotropic_scenes(w, h, n, seed):
    _pin(F.anisotropic(w, h, n, seed), f"anisotropic {w}x{h} N={n}", min_rendered=n // 2)


@needs_reference
def test_trained_like_pose():
    ref = _pin(F.trained_like_pose(), "trained-like pose", min_rendered=5000)
    assert int(ref["tilesTouched"].max()) >= 100                # (the background splats)


@needs_reference
def test_equal_keys_keep_index_order():
    ref = _pin(F.equal_keys(), "equal keys")
    same = ref["keys"][1:] == ref["keys"][:-1]
    assert same.sum() >= 2000 and bool((ref["values"][1:][same] > ref["values"][:-1][same]).all())


@needs_reference
def test_opaque_stack_past_the_first_round():
    ref = _pin(F.opaque_stack(), "opaque stack")
    lengths = ref["ranges"][:, 1].astype(np.int64) - ref["ranges"][:, 0]
    assert int(lengths.max()) > 256                                          # records past the first 256-entry round
    assert int(ref["nContrib"].min()) < 256 < int(ref["nContrib"].max())     # pixels that stop early, pixels that go on
    assert float(ref["finalT"].min()) < 0.01


@needs_reference
def test_single_instance_draws_nothing():
    """R == 1: identifyTileRanges (GSCuda.cu:515-537) opens the only tile and never closes it: the picture is the background."""
    scene, cam, bg, kw = F.single_instance()
    ref = _pin((scene, cam, bg, kw), "R == 1")
    assert ref["num_rendered"] == 1 and ref["keys"].size == 1
    assert not ref["ranges"].any()
    assert np.array_equal(ref["out_color"], np.broadcast_to(np.asarray(bg, np.float32)[:, None, None], (3, 64, 64)))
    assert (ref["finalT"] == 1.0).all() and not ref["nContrib"].any()


@needs_reference
def test_nothing_rendered_returns_before_the_binning_allocator():
    """R == 0 (GSCuda.cu:775-778): out_color keeps what it held, the binning allocator is not called, nothing of the image
    state is written."""
    scene, cam, bg, kw = F.nothing_visible()
    ref = _pin((scene, cam, bg, kw), "R == 0", min_rendered=0)
    assert ref["num_rendered"] == 0 and ref["alloc_calls"] == (1, 1, 0)
    assert (ref["out_color"] == 0.25).all()
    assert not ref["finalT"].any() and not ref["nContrib"].any() and not ref["ranges"].any()
    for name, got in _oracles(scene, cam, bg, kw):
        assert (got["out_color"] == 0.25).all(), name


@needs_reference
@pytest.mark.parametrize("modifier", [0.37, 2.5])
def test_scale_modifier(modifier):
    ref = _pin(F.scale_modified(modifier), f"scale_modifier {modifier}")
    base = ref_cpu.forward(*F.anisotropic(200, 120, 3000, 7)[:3])
    assert not np.array_equal(ref["cov3D"], base["cov3D"])


@needs_reference
def test_quaternions_far_from_unit_length():
    _pin(F.far_from_unit_quaternions(), "quaternions far from unit length")


@needs_reference
def test_opacities_zero_one_above_and_below():
    frame = F.odd_opacities()
    ref = _pin(frame, "opacities 0, 1, 2, -0.5, 1e-9")
    seen = ref["conicOpacity"][ref["tilesTouched"] > 0, 3]
    for v in (0.0, 1.0, 2.0, -0.5):
        assert (seen == np.float32(v)).any(), v


@needs_reference
def test_splats_on_the_camera_plane():
    frame = F.on_camera_plane()
    scene, cam = frame[0], frame[1]
    w_clip = (np.asarray(cam.proj, np.float64).reshape(4, 4).T @ scene["means3D"].astype(np.float64).T)[3]
    assert int((np.abs(w_clip) < 1e-6).sum()) >= 100            # clip w = 0: the 0.001 of GSCuda.cu:304 alone divides
    _pin(frame, "splats on the camera plane")


@needs_reference
@pytest.mark.parametrize("colors,cov3d", [(True, False), (False, True), (True, True)])
def test_precomputed_colours_and_covariances(colors, cov3d):
    scene, cam, bg, kw = F.precomputed_inputs(colors, cov3d)
    ref = _pin((scene, cam, bg, kw), f"colorsPrecomp={colors} cov3DPrecomp={cov3d}")
    assert ref["rgb"].any() == (not colors) and ref["cov3D"].any() == (not cov3d)      # (not written when given)
    plain = ref_cpu.forward(scene, cam, bg)
    assert not np.array_equal(plain["out_color"], ref["out_color"])


@needs_reference
def test_callers_radii_or_the_states_own():
    """radii == nullptr (GSCuda.cu:726-729): GeometryState::internalRadii takes the radii; with a caller's array it stays
    untouched. Everything else is the same call."""
    scene, cam, bg, kw = F.anisotropic(64, 48, 500, 3)
    own = ref_cpu.forward(scene, cam, bg, callers_radii=True)
    internal = ref_cpu.forward(scene, cam, bg, callers_radii=False)
    assert own["radii"].any() and not own["internalRadii"].any()
    assert np.array_equal(internal["internalRadii"], own["radii"])
    assert not _differing(own, internal)
    for name, got in _oracles(scene, cam, bg, kw):
        assert not _differing(internal, got), name


@needs_reference
def test_grid_wider_than_255_tile_columns():
    """4112 x 40 -> 257 x 3 tiles: tile ids beyond one byte (the recipe of test_gpu_parity; it reaches 52 tile columns)."""
    ref = _pin(F.wide_grid(), "4112 x 40 (257 tile columns)", min_rendered=1000)
    assert int((ref["keys"] >> np.uint64(32)).max()) > 255


@needs_reference
def test_grid_wider_than_255_tile_columns_with_splats_in_the_last_columns():
    ref = _pin(F.wide_grid_all_columns(), "4112 x 40, every tile column", min_rendered=1000)
    columns = (ref["keys"] >> np.uint64(32)) % np.uint64(257)
    assert int(columns.max()) == 256 and int(columns.min()) == 0 and np.unique(columns).size > 240


@needs_reference
@pytest.mark.parametrize("near,extra", F.DEPTH_KEY_CASES)
def test_depth_keys_outside_the_main_top_byte(near, extra):
    ref = _pin(F.depth_keys(near, extra), f"depth keys, near={near} extra={extra}")
    vis = ref["tilesTouched"] != 0
    others = int(((ref["depths"].view(np.uint32)[vis] >> 24) != 0x3F).sum())
    nvis = int(vis.sum())
    assert {(0.5, 12): 2 <= others <= 16, (0.5, 1): 1 <= others <= 3, (1.3, 0): 1024 < others < nvis, (3.0, 0): others == nvis,
            (0.01, 0): others == 0}[(near, extra)], (others, nvis)


# ---------------------------------------------------------------- extreme inputs
@needs_reference
@pytest.mark.parametrize("seed", range(10))
def test_extreme_inputs_with_every_conversion_in_range(seed):
    """The extreme_but_finite recipe (1e-8 scales, 1e6 : 1 needles, quaternions far from unit length, odd opacities, splats on
    the camera plane and 1e5 units away, an eye inside the cloud) with the two scale factors bounded (reference_frames.
    EXTREME_BOUNDED) so that every float -> int conversion of the reference stays inside int — asserted from the reference's
    own outputs by _pin (conversions_in_range). Each of the ten frames still has splats whose rectangle exceeds the screen,
    so the clamps of getRect are exercised."""
    frame = F.extreme_but_finite(seed, **F.EXTREME_BOUNDED)
    cam = frame[1]
    ref = _pin(frame, f"extreme, in range, seed {seed}")
    vis = ref["tilesTouched"] > 0
    beyond = vis & ((ref["rects"][:, 0] > cam.width) | (ref["rects"][:, 1] > cam.height))
    assert beyond.any(), "no splat whose rect exceeds the screen"
    whole = vis & (ref["tilesTouched"] == ((cam.width + 15) // 16) * ((cam.height + 15) // 16))
    print(f"[reference pin] seed {seed}: {int(beyond.sum())} rects beyond the screen, {int(whole.sum())} cover every tile, "
          f"largest extent {int(ref['rects'].max())}")


@needs_reference
def test_out_of_range_conversions_are_the_only_difference_left():
    """The unbounded extreme_but_finite recipe (tests/test_gpu_parity.py's): screen-filling splats whose
    (int) ceil(3.0f * cov.z) (GSCuda.cu:352) leaves int. There the host build of the reference and the oracles MUST differ:
    the conversion is undefined on the host (x86 yields INT_MIN) and saturates on the device (INT_MAX), which is what the
    oracles state. No host build can pin these inputs: DEVICE SATURATION THERE IS PINNED BY THE ORACLE'S STATEMENT OF THE
    CONVERSION ALONE (gsr_oracle.cpp f2i, oracle_np._f2i), and the GPU suite's extreme frames rest on it.
    Shown here, over the ten seeds: (1) every Gaussian with any differing per-Gaussian output has an out-of-range conversion —
    seen in the oracle's own saturated extents AND in the reference's; (2) every other Gaussian's preprocess outputs are byte-
    equal; (3) with the reference's extents of exactly those Gaussians replaced by the saturated ones, its rectangles give
    the oracle's tile counts: the difference is the conversion and what follows from it, nothing else; (4) frames without such
    a Gaussian are byte-equal in every output."""
    differing_frames, clean_frames, culprits = 0, 0, 0
    for seed in range(10):
        scene, cam, bg, kw = F.extreme_but_finite(seed, **F.EXTREME_UNBOUNDED)
        ref = ref_cpu.forward(scene, cam, bg, **kw)
        assert ref["num_rendered"] > 0
        exp = cpu_oracle.forward(scene, cam, bg, **kw)
        assert not _differing(exp, oracle_np.forward(scene, cam, bg, exp=cpu_oracle.expf, **kw)), "the two oracles agree on saturation"
        n = scene["means3D"].shape[0]
        differs = np.zeros(n, bool)
        for k in F.PREPROCESS_KEYS:
            a, b = np.ascontiguousarray(ref[k]).reshape(n, -1), np.ascontiguousarray(exp[k]).reshape(n, -1)
            differs |= (a.view(np.uint8) != b.view(np.uint8)).any(1)
        saturated = (exp["rects"] == F.INT_MAX).any(1) | (exp["radii"] == F.INT_MAX)         # the oracle's statement of the device
        out_of_range = ~F.conversions_in_range(ref, cam)                                     # the reference's own outputs
        assert not (differs & ~saturated).any() and not (differs & ~out_of_range).any(), (seed, np.nonzero(differs & ~saturated)[0][:8])
        assert np.array_equal(saturated, out_of_range), seed
        if not differs.any():
            assert not _differing(ref, exp), seed
            clean_frames += 1
            continue
        differing_frames += 1
        culprits += int(differs.sum())
        # (3) what does not depend on the rectangle is equal for the culprits too: cov3D (written before the conversion), the
        # extent that stayed in range, and - where both sides keep the Gaussian - radius, centre, depth, conic and colour; the
        # extent that left int is INT_MIN here and INT_MAX in the oracle, and getRect restated over the reference's own extents
        # with exactly those saturated gives the oracle's tile counts
        assert _bytes_equal(ref["cov3D"], exp["cov3D"]), seed
        a, b = ref["rects"].astype(np.int64), exp["rects"].astype(np.int64)
        assert (((a == b) | ((a == F.INT_MIN) & (b == F.INT_MAX)))).all(), seed
        both = saturated & (ref["tilesTouched"] > 0) & (exp["tilesTouched"] > 0)
        for k in ("radii", "means2D", "depths", "conicOpacity", "rgb"):
            assert _bytes_equal(ref[k][both], exp[k][both]), (seed, k)
        kept = saturated & (exp["tilesTouched"] > 0)
        ext = np.where(a == F.INT_MIN, F.INT_MAX, a).astype(np.int32)
        gx, gy = (cam.width + 15) // 16, (cam.height + 15) // 16
        m = exp["means2D"]
        x0, y0, x1, y1 = oracle_np._rect(m[:, 0], m[:, 1], ext[:, 0], ext[:, 1], gx, gy)
        tiles = ((x1 - x0) * (y1 - y0)).astype(np.uint32)
        assert kept.any() and np.array_equal(tiles[kept], exp["tilesTouched"][kept]), seed
    print(f"[reference pin] unbounded extremes: {differing_frames} frames differ ({culprits} Gaussians, all with an out-of-range "
          f"conversion), {clean_frames} frames byte-equal")
    assert differing_frames >= 5 and clean_frames >= 1          # (the recipe does reach the conversion, and not in every frame)


# ---------------------------------------------------------------- forwardPoints, getHigherMsb, the chunk layouts
@needs_reference
@pytest.mark.parametrize("w,h,n,seed", [(64, 48, 400, 3), (333, 257, 200_000, 5), (1920, 1080, 2_000_000, 9)])
def test_forward_points_against_the_numpy_restatement(w, h, n, seed):
    """gscuda::forwardPoints on the scenes of tests/test_points.py. Where several points land on one pixel the reference's
    outcome depends on the order its threads run in (atomicMin, then an unordered colour write). The host build runs them in
    index order: the nearest point wins and, among equal depths, the lowest index — the rule oracle/points_np.py states and
    the HIP path implements. Depth ties do occur in these scenes and are decided by that rule on both sides."""
    from gsrast_amd import camera, scenes
    cam = camera.default_camera(w, h)
    sc = scenes.garden_like_scene(n, seed=seed)
    sc["means3D"][:, :3] *= 0.3
    if n == 400:                                                    # (test_points_oracle_basics' three placed points)
        sc["means3D"][0, :3] = (0.0, 0.0, -4.5); sc["means3D"][1, :3] = (0.0, 0.0, -4.0); sc["means3D"][2, :3] = (0.0, 0.0, -50.0)
    bg = (0.1, 0.2, 0.3)
    exp_out, exp_depth = points_np.forward_points(sc["means3D"][:, :3], sc["shs"], cam.proj, w, h, bg)
    out, depth = ref_cpu.forward_points(sc["means3D"][:, :3], sc["shs"], cam.proj, w, h, bg)
    assert (depth != 1.0).sum() > min(n, w * h) // 20
    assert _bytes_equal(depth, exp_depth) and _bytes_equal(out, exp_out)
    calls, sizes = ref_cpu.forward_points.last_alloc
    assert calls == (1, 0, 1) and sizes[0] == 32 and sizes[2] == ref_cpu.required("points_image", w * h) + 32     # GSCuda.cu:127-134


@needs_reference
def test_higher_msb_three_ways():
    from gsrast_amd import _capi
    L = _capi.lib()
    edge = sorted({v for k in range(33) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if 0 <= v < (1 << 32)})
    assert edge[-1] == (1 << 32) - 1
    for n in list(range(0, (1 << 17) + 1)) + edge:
        want = ref_cpu.higher_msb(n)
        assert L.gsr_higher_msb(n) == want == cpu_oracle.higher_msb(n), n
        assert oracle_np.higher_msb(n) == want, n


@pytest.fixture
def temp_sizes():
    """Lets a test set the scan / sort temporary sizes the cub stand-in reports, and puts the defaults back."""
    yield ref_cpu.set_temp_sizes
    ref_cpu.set_temp_sizes()


BASES = [0, 1 << 20, (1 << 20) + 4, (1 << 20) + 37, (1 << 20) + 127, (1 << 33) + 129]


@needs_reference
@pytest.mark.parametrize("n", [1, 1000, 5_834_784])
def test_geometry_chunk_layout_is_the_references(n, temp_sizes):
    """gs::GeometryState::fromChunk (AuxBuffer.cu:44-63) itself against gsr_geometry_from_chunk, on aligned and unaligned
    bases. scanSize is whatever the scan asks for: CUB's number there, this library's own scratch here (not less than
    gsr_scan_temp_bytes). The stand-in's scan is told to ask for this library's size; every pointer must then agree."""
    from gsrast_amd import _capi
    L = _capi.lib()
    st = _capi.GeometryState()
    L.gsr_geometry_from_chunk(0, n, C.byref(st))
    assert st.scan_size >= L.gsr_scan_temp_bytes(n)
    temp_sizes(st.scan_size, 1)
    for base in BASES:
        end = L.gsr_geometry_from_chunk(base, n, C.byref(st))
        ref = ref_cpu.from_chunk("geometry", base, n)
        got = dict(tilesTouched=st.tiles_touched, scanSize=st.scan_size, scanningSpace=st.scanning_space, depths=st.depths,
                   clamped=st.clamped, internalRadii=st.internal_radii, means2D=st.means2D, cov3D=st.cov3D,
                   conicOpacity=st.conic_opacity, rgb=st.rgb, pointOffsets=st.point_offsets, end=end)
        assert {k: (v or 0) for k, v in got.items()} == ref, (n, base)
    assert L.gsr_required_geometry(n) == ref_cpu.required("geometry", n)


@needs_reference
@pytest.mark.parametrize("pixels,records", [(1920 * 1080, 1_000_003), (1, 1), (333 * 257, 1000), (64 * 64 + 1, 5_834_784)])
def test_image_and_binning_chunk_layouts_are_the_references(pixels, records, temp_sizes):
    """gs::ImageState / gs::BinningState::fromChunk (AuxBuffer.cu:65-89) against gsr_image_from_chunk / gsr_binning_from_chunk;
    sortingSize as scanSize above (this library's is not less than gsr_sort_temp_bytes)."""
    from gsrast_amd import _capi
    L = _capi.lib()
    b = _capi.BinningState()
    L.gsr_binning_from_chunk(0, records, C.byref(b))
    assert b.sorting_size >= L.gsr_sort_temp_bytes(records)
    temp_sizes(1, b.sorting_size)
    for base in BASES:
        im = _capi.ImageState()
        end = L.gsr_image_from_chunk(base, pixels, C.byref(im))
        got = dict(ranges=im.ranges, nContrib=im.n_contrib, accumAlpha=im.accum_alpha, end=end)
        assert {k: (v or 0) for k, v in got.items()} == ref_cpu.from_chunk("image", base, pixels), (pixels, base)
        end = L.gsr_binning_from_chunk(base, records, C.byref(b))
        ref = ref_cpu.from_chunk("binning", base, records)
        got = dict(pointListKeysUnsorted=b.keys_unsorted, pointListKeys=b.keys, pointListUnsorted=b.values_unsorted,
                   pointList=b.values, sortingSize=b.sorting_size, listSortingSpace=b.sorting_space, end=end)
        assert {k: (v or 0) for k, v in got.items()} == ref, (records, base)
    assert L.gsr_required_image(pixels) == ref_cpu.required("image", pixels)
    assert L.gsr_required_binning(records) == ref_cpu.required("binning", records)


@needs_reference
def test_points_image_chunk_layout_is_the_references():
    """pc::ImageState (AuxBuffer.cu:31-39); this library carves one more array (the winners) behind the reference's three."""
    from gsrast_amd import _capi
    L = _capi.lib()
    for base in BASES:
        for pixels in (1, 1000, 1920 * 1080):
            st = _capi.PointsImageState()
            L.gsr_points_image_from_chunk(base, pixels, C.byref(st))
            ref = ref_cpu.from_chunk("points_image", base, pixels)
            assert ((st.depth or 0), st.out_color, st.default_depth) == (ref["depth"], ref["outColor"], ref["defaultDepth"])
            assert ref["end"] == ref["defaultDepth"] + 4 <= st.winner
    assert ref_cpu.required("points_geometry", 1000) == 0


# ---------------------------------------------------------------- the committed fixture
def _fixture_frames():
    z = np.load(FIXTURE)
    names = [str(s) for s in z["frames"]]
    from gsrast_amd.camera import Camera
    for name in names:
        g = lambda k: z[f"{name}/{k}"]
        n = g("in_means3D").shape[0]
        shs = np.zeros((n, 48), np.float32)
        shs[:, :3] = g("in_shs_dc")
        scene = {"means3D": g("in_means3D"), "scales": g("in_scales"), "rotations": g("in_rotations"), "opacities": g("in_opacities"),
                 "shs": shs}
        cam = Camera(view=g("cam_view"), proj=g("cam_proj"), cam_pos=g("cam_pos"), tan_fovx=float(g("cam_tan")[0]),
                     tan_fovy=float(g("cam_tan")[1]), width=int(g("size")[0]), height=int(g("size")[1]))
        kw = dict(use_rects=bool(g("use_rects")), scale_modifier=float(g("scale_modifier")))
        for k in ("colors_precomp", "cov3d_precomp", "out_init"):
            if f"{name}/in_{k}" in z.files:
                kw[k] = g("in_" + k)
        exp = {k: (g("exp_" + k) if f"{name}/exp_{k}" in z.files else None) for k in F.REF_KEYS}
        exp["num_rendered"] = int(g("num_rendered"))
        yield name, scene, cam, tuple(float(v) for v in g("background")), kw, exp


def test_oracles_against_the_recorded_reference_frames():
    """tests/golden/reference_frames.npz: outputs recorded from the reference binary (tests/golden/make_reference_frames.py).
    Runs anywhere, with or without the binary: both oracles byte for byte against the record."""
    assert os.path.getsize(FIXTURE) <= 297 * 1024
    count = 0
    for name, scene, cam, bg, kw, exp in _fixture_frames():
        for oracle_name, got in _oracles(scene, cam, bg, kw):
            bad = _differing(exp, got)
            assert not bad, f"{name}: {oracle_name} differs from the recorded reference outputs in {bad}"
        count += 1
    assert count >= 5


@needs_reference
def test_recorded_reference_frames_are_what_the_binary_gives_now():
    """A stale fixture (the reference, the stand-ins or the recipe moved) fails here."""
    for name, scene, cam, bg, kw, exp in _fixture_frames():
        ref = ref_cpu.forward(scene, cam, bg, **kw)
        bad = _differing(exp, ref)
        assert not bad, f"{name}: the fixture no longer matches the reference binary in {bad}; re-mint it"
