"""The `inria` semantics profile: upstream diff-gaussian-rasterization semantics
behind the same boundary. Unpinned by the reference; the HIP path is checked against this repo's
numpy restatement (oracle/inria_np.py) and closed-form facts. What can be pinned of the restatement without the upstream
text is pinned here on the CPU: its sixteen polynomials are the real spherical harmonics, its float32 colour is the float64
one of oracle/backward_np.py, its two blends agree, and it never counts an instance it does not emit. The GPU side of the
profile is in tests/test_gpu_inria_parity.py."""
import numpy as np
import pytest

from helpers import single_gaussian_scene, inria_scene, opaque_stack_scene, stop_census, run_inria, compare_inria
from gsrast_amd import camera, scenes
from oracle import inria_np


_scene = inria_scene


def test_sh_basis_closed_forms():
    """Degree 0 is view independent: colour = SH_C0 * dc + 0.5; degree 1 along +z adds SH_C1 * sh[2]."""
    pos = np.array([[0.0, 0.0, 2.0]], np.float32)
    cam = np.zeros(3, np.float32)
    shs = np.zeros((1, 48), np.float32)
    shs[0, 0:3] = (1.0, -4.0, 0.5)
    shs[0, 6:9] = (0.2, 0.2, 0.2)            # coefficient 2 (the z term of degree 1)
    rgb0, clamped0 = inria_np.sh_to_rgb(0, pos, cam, shs)
    assert np.allclose(rgb0[0], np.maximum(0.28209479 * shs[0, 0:3] + 0.5, 0), atol=1e-6) and clamped0[0, 1]
    rgb1, _ = inria_np.sh_to_rgb(1, pos, cam, shs)
    assert np.allclose(rgb1[0, 0] - rgb0[0, 0], 0.48860251 * 0.2, atol=1e-6)


def _recovered_basis(dirs):
    """Basis function k of inria_np.sh_to_rgb at the unit directions `dirs`: coefficient +-0.25 e_k gives the colours
    0.5 +- 0.25 Y_k (|Y_k| < 1.1: neither is clamped), their difference divided by 0.5 is Y_k. float32 throughout."""
    pos, cam = dirs.astype(np.float32), np.zeros(3, np.float32)
    out = np.zeros((16, len(dirs)))
    for k in range(16):
        shs = np.zeros((len(dirs), 48), np.float32)
        shs[:, 3 * k] = 0.25
        plus, cp = inria_np.sh_to_rgb(3, pos, cam, shs)
        minus, cm = inria_np.sh_to_rgb(3, pos, cam, -shs)
        assert not cp.any() and not cm.any()
        out[k] = (plus[:, 0].astype(np.float64) - minus[:, 0].astype(np.float64)) / 0.5
    return out


def test_sh_basis_is_the_real_spherical_harmonics_in_the_standard_order():
    """The sixteen functions of the restatement, projected on the real spherical harmonics built from scipy's complex ones
    (k = l^2 + l + m; sqrt2 (-1)^m Im Y_l^|m| for m < 0, Y_l^0, sqrt2 (-1)^m Re Y_l^m for m > 0) on a Gauss-Legendre x
    uniform-phi grid of 12 x 24 nodes, which integrates products of two cubics exactly: the matrix is diagonal with entries
    (-1)^k (the published basis carries that sign convention). Bound 5e-6 on the off-diagonal entries and on | |diagonal| - 1 |:
    a recovered value is the difference of two float32 colours of magnitude at most 1, each about ten float32 operations
    (10 * 2^-24 = 6e-7), divided by 0.5: 2.4e-6 pointwise at most, integrated against a function whose square integrates to
    one (Cauchy-Schwarz with sqrt(4 pi): 8.5e-6 at the very worst, and the errors do not line up). A constant wrong in its fifth
    digit (1e-5 relative) fails, two swapped polynomials or a flipped sign fail outright. Without scipy the Gram matrix of
    the sixteen alone must be the identity within 1e-5 (the same derivation, two recovered factors): that pins constants and
    polynomials, not their order or sign."""
    mu, w_mu = np.polynomial.legendre.leggauss(12)
    phi = (np.arange(24) + 0.5) * (2.0 * np.pi / 24)
    MU, PHI = np.meshgrid(mu, phi, indexing="ij")
    wgt = (w_mu[:, None] * np.full((1, 24), 2.0 * np.pi / 24)).reshape(-1)
    st = np.sqrt(1.0 - MU * MU)
    dirs = np.stack([st * np.cos(PHI), st * np.sin(PHI), MU], axis=-1).reshape(-1, 3)
    Y = _recovered_basis(dirs)
    try:
        from scipy.special import sph_harm_y
    except ImportError:
        sph_harm_y = None
    if sph_harm_y is None:
        gram = (Y * wgt) @ Y.T
        worst = float(np.abs(gram - np.eye(16)).max())
        print(f"[sh basis] no scipy: Gram matrix of the sixteen functions, max |G - I| = {worst:.2e}")
        assert worst <= 1e-5
        return
    theta = np.arccos(MU).reshape(-1)
    ref = np.zeros((16, dirs.shape[0]))
    for l in range(4):
        for m in range(-l, l + 1):
            c = sph_harm_y(l, abs(m), theta, PHI.reshape(-1))
            ref[l * l + l + m] = (c.real if m == 0 else np.sqrt(2.0) * (-1) ** m * (c.imag if m < 0 else c.real))
    proj = (Y * wgt) @ ref.T
    diag = np.diag(proj)
    off = proj - np.diag(diag)
    print(f"[sh basis] scipy: worst off-diagonal {float(np.abs(off).max()):.2e}, worst | |diagonal| - 1 | {float(np.abs(np.abs(diag) - 1).max()):.2e}, "
          f"signs {''.join('+' if v > 0 else '-' for v in diag)}")
    assert np.array_equal(np.sign(diag), np.array([(-1.0) ** k for k in range(16)]))
    assert float(np.abs(off).max()) <= 5e-6 and float(np.abs(np.abs(diag) - 1.0).max()) <= 5e-6


# float32 operations on the way to one colour channel, per degree, for the standard bound of a float32 sum of products: the
# unit direction costs six roundings per component (subtraction, square, two additions, root, division) and enters a term
# of degree l to the l-th power (6 l); then the longest term of the band — degree 3: SH_C3[3] z (2 zz - 3 xx - 3 yy) sh, three
# scalings, two subtractions, three products = 8; degree 2: SH_C2[2] (2 zz - xx - yy) sh = 6 (zz, the scaling, two
# subtractions, two products); degree 1: two products; degree 0: one —, the rounding of its float32 constant (1), and one
# addition per term that follows, the 0.5 included ((l + 1)^2 of them).
_SH_OPS = {0: 0 + 1 + 1 + 1, 1: 6 + 2 + 1 + 4, 2: 12 + 6 + 1 + 9, 3: 18 + 8 + 1 + 16}


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_float32_colour_against_the_float64_one(deg):
    """inria_np.sh_to_rgb (float32, the kernel's expression) against backward_np's float64 colour on 2 000 random (position,
    camera, coefficients). Bound per sample, in float64 from the sample itself: 2^-24 ops (0.5 + sum_k |Y_k(d)| |c_k|), the
    standard bound of a float32 sum of products against its exact value (ops: _SH_OPS above; 43 at degree 3). The clamp flags
    agree wherever the float64 value is further from zero than that bound."""
    from oracle import backward_np as B
    rng = np.random.default_rng(100 + deg)
    n = 2000
    pos = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    cam = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    shs = rng.normal(0, 0.3, (n, 48)).astype(np.float32)
    worst, worst_ratio, flags = 0.0, 0.0, 0
    assert _SH_OPS[3] in range(40, 50)
    for i in range(n):
        got, clamped = inria_np.sh_to_rgb(deg, pos[i:i + 1], cam[i], shs[i:i + 1])
        v = pos[i].astype(np.float64) - cam[i].astype(np.float64)
        basis, _ = B.sh_basis(v / np.linalg.norm(v), deg)
        c = shs[i].astype(np.float64).reshape(16, 3)
        raw = basis @ c + 0.5
        bound = 2.0 ** -24 * _SH_OPS[deg] * (0.5 + np.abs(basis) @ np.abs(c))
        err = np.abs(got[0].astype(np.float64) - np.maximum(raw, 0.0))
        assert (err <= bound).all(), (i, err, bound)
        assert np.allclose(np.maximum(raw, 0.0), B.inria_color(pos[i], cam[i], c, deg), rtol=0, atol=1e-15)
        sure = np.abs(raw) > bound
        assert np.array_equal(clamped[0][sure], (raw < 0)[sure]), i
        flags += int(clamped.sum())
        worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / bound).max()))
    print(f"[sh colour] degree {deg}: worst |float32 - float64| {worst:.2e}, worst share of the bound {worst_ratio:.2f}, {flags} clamped channels")
    assert flags > 0 or deg == 0          # (degree 0 with N(0, 0.3) coefficients: a clamp is a six-sigma event)


def test_the_two_blends_of_the_restatement_agree_at_the_cutoff():
    """oracle_np.blend given libm's expf (cpu_oracle.expf) and the C++ tile loop with t_cutoff = 1e-4 give the same nContrib
    and finalT words (and pixels) on a frame with opaque stacks — pixels that stop at 1e-4, and pixels that would have
    stopped at 1e-3 and do not; the C++ loop at its default cut-off decides differently on that frame."""
    from oracle import cpu_oracle
    sc = opaque_stack_scene()
    cam = camera.default_camera(160, 96, near=0.05, far=50.0)
    bg = (0.1, 0.2, 0.3)
    a = inria_np.forward(sc, cam, bg, blend_with="numpy-expf")
    b = inria_np.forward(sc, cam, bg, blend_with="cpp", threads=4)
    stop4, stop3_only = stop_census(b, cam)
    print(f"[blends] {stop4} pixels stop at 1e-4, {stop3_only} more would have stopped at 1e-3")
    assert stop4 > 100 and stop3_only > 100
    assert np.array_equal(a["nContrib"], b["nContrib"])
    assert np.array_equal(a["finalT"].view(np.uint32), b["finalT"].view(np.uint32))
    assert np.array_equal(a["out_color"].view(np.uint32), b["out_color"].view(np.uint32))
    assert a["records_staged"] == b["records_staged"]
    c = cpu_oracle.blend_cutoff(b, cam, bg, threads=1, t_cutoff=0.001)
    assert (c["nContrib"] != b["nContrib"]).sum() >= stop3_only and (c["nContrib"] <= b["nContrib"]).all()


def overflow_ladder():
    """(scales, quaternion factors) of the Gaussians a diverged trainer produces: every value finite in float32, the
    covariance overflowing somewhere along the ladder."""
    return [10.0 ** e for e in range(4, 20)], [10.0 ** e for e in range(3, 11)]


def ladder_scene(n=400, seed=9):
    """Ordinary Gaussians, and in front of the camera one per step of overflow_ladder(); returns (scene, ids of those)."""
    sc = inria_scene(n, seed)
    scales, factors = overflow_ladder()
    ids = np.arange(10, 10 + 7 * (len(scales) + len(factors)), 7)
    rng = np.random.default_rng(seed)
    sc["means3D"][ids, :3] = rng.uniform(-0.4, 0.4, (len(ids), 3))
    for j, s in enumerate(scales):
        sc["scales"][ids[j], :3] = s
    for j, f in enumerate(factors):
        sc["rotations"][ids[len(scales) + j]] *= np.float32(f)
    sc["opacities"][ids] = 0.9
    return sc, ids


def test_restatement_counts_what_it_emits_on_the_overflow_ladder():
    """Scales 1e4 .. 1e19 and quaternions x 1e3 .. 1e10 (this profile does not normalise them): the sum of tilesTouched,
    num_rendered and the number of keys agree, no Gaussian has a tile with radius 0 or a non-finite conic, and some steps of
    the ladder do overflow (no tile in front of the camera, in the middle of the frame)."""
    cam = camera.default_camera(200, 120, near=0.05, far=50.0)
    sc, ids = ladder_scene()
    assert np.isfinite(sc["scales"]).all() and np.isfinite(sc["rotations"]).all()
    o = inria_np.forward(sc, cam, (0.1, 0.2, 0.3), blend_with="cpp")
    assert int(o["tilesTouched"].astype(np.int64).sum()) == o["num_rendered"] == o["keys"].size
    has = o["tilesTouched"] > 0
    assert (o["radii"][has] > 0).all() and not (o["radii"][~has] != 0).any()
    assert np.isfinite(o["conicOpacity"][has]).all() and np.isfinite(o["out_color"]).all()
    lost = ids[~has[ids]]
    print(f"[ladder] {len(lost)} of {len(ids)} ladder Gaussians have no tile: {lost.tolist()}")
    assert 0 < len(lost) < len(ids)
    for s in (1e15, 1e19):                       # one Gaussian alone, as it was first found
        one = single_gaussian_scene(pos=(0.0, 0.0, 0.0), scale=s, n=1)
        o1 = inria_np.forward(one, cam, blend_with="cpp")
        assert o1["num_rendered"] == o1["keys"].size == int(o1["tilesTouched"].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n,seed,deg", [(200, 120, 3000, 7, 3), (128, 128, 1500, 3, 1), (333, 257, 8000, 11, 2), (64, 48, 400, 5, 0)])
def test_inria_profile_matches_numpy_restatement(w, h, n, seed, deg):
    from gsrast_amd.rasterizer import SplatRasterizer
    sc = _scene(n, seed)
    cam = camera.default_camera(w, h, near=0.05, far=50.0)
    bg = (0.1, 0.2, 0.3)
    exp = inria_np.forward(sc, cam, bg, deg=deg, blend_with="cpp", threads=4)
    r, img = run_inria(sc, cam, bg, sh_degree=deg)
    # every output, bit for bit but the pixels (helpers.PIXEL_TOL): tests/test_gpu_inria_parity.py has the other cases
    compare_inria(r, img, exp, f"{w}x{h} N={n} deg={deg} plan={r.last_plan}")
    # and it really is a different renderer than the gscuda semantics
    img_gs = r.draw(cam).cpu().numpy()
    assert np.abs(img_gs - img).max() > 1e-2


@pytest.mark.gpu
def test_inria_edge_cases_background_and_single_instance():
    from gsrast_amd.rasterizer import SplatRasterizer
    cam = camera.default_camera(64, 64)
    bg = (0.2, 0.3, 0.4)
    r = SplatRasterizer(64, 64, background=bg)
    r.configure_from_scene(single_gaussian_scene(pos=(0, 0, -50.0), n=3))       # nothing visible
    r.out_color.fill_(0.9)
    img = r.draw(cam, semantics="inria").cpu().numpy()
    assert r.last_num_rendered == 0
    assert np.allclose(img[0], 0.2) and np.allclose(img[2], 0.4)                # upstream still writes the background
    one = single_gaussian_scene(pos=(0.5178, -0.5178, 0.0), scale=0.001, n=1)
    exp = inria_np.forward(one, cam, bg, deg=0, blend_with="cpp")
    r, img = run_inria(one, cam, bg, sh_degree=0)
    assert r.last_num_rendered == exp["num_rendered"] >= 1
    compare_inria(r, img, exp, "a single instance")
    assert np.abs(img[0] - 0.2).max() > 1e-3                                     # the single instance IS drawn (D12)
