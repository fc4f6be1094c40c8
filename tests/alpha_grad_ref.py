"""The reference of the accumulated opacity's gradient (gsr_backward_alpha, include/gsrast_amd_opacity.h), float64, from the oracle as it is.

out_alpha = 1 - finalT = sum_i alpha_i T_i is what the blend loop gives for colours (1, 0, 0) over a black background in
channel 0, so the term sum_p g_a (1 - finalT) of the loss has the per-Gaussian gradients of oracle.backward_np.blend_backward
called with those colours, that background and dL_dout = (g_a, 0, 0): its dL_dmean2D, dL_dconic and dL_dopacity (its
dL_dcolor belongs to the colours that were put in, not to the scene's: the opacity does not depend on them). The full
reference adds the ordinary colour call — the superposition tests/test_gpu_depth_backward.py uses for the depth channel."""
import numpy as np

from oracle import backward_np as B

GEOMETRY = ("dL_dmean2D", "dL_dconic", "dL_dopacity")


def alpha_term(means2D, conic_opacity, ranges, point_list, n_contrib, final_t, width, height, g_alpha):
    """Per-Gaussian gradients of sum(g_alpha * (1 - finalT)): {dL_dmean2D [N,2], dL_dconic [N,3], dL_dopacity [N]}."""
    n = np.asarray(means2D).shape[0]
    ones = np.zeros((n, 3))
    ones[:, 0] = 1.0
    g3 = np.zeros((3, height, width))
    g3[0] = np.asarray(g_alpha, np.float64)
    res = B.blend_backward(means2D, conic_opacity, ones, ranges, point_list, n_contrib, final_t, width, height, (0.0, 0.0, 0.0), g3)
    return {k: res[k] for k in GEOMETRY}


def superposed(means2D, conic_opacity, colors, ranges, point_list, n_contrib, final_t, width, height, background, dL_dout, g_alpha):
    """(full, alpha term): the colour call's gradients plus the alpha term's; dL_dcolor is the colour call's alone."""
    col = B.blend_backward(means2D, conic_opacity, colors, ranges, point_list, n_contrib, final_t, width, height, background, dL_dout)
    term = alpha_term(means2D, conic_opacity, ranges, point_list, n_contrib, final_t, width, height, g_alpha)
    full = {k: col[k] + term[k] for k in GEOMETRY}
    full["dL_dcolor"] = col["dL_dcolor"]
    return full, term


def alpha_loss(means2D, conic_opacity, ranges, point_list, width, height, g_alpha, t_cutoff):
    """sum(g_alpha * (1 - finalT)) of blend_forward: what the finite differences are taken of."""
    col = np.zeros((np.asarray(means2D).shape[0], 3))
    ft = B.blend_forward(means2D, conic_opacity, col, ranges, point_list, width, height, (0.0, 0.0, 0.0), t_cutoff=t_cutoff)[1]
    return float((np.asarray(g_alpha, np.float64) * (1.0 - ft)).sum())


def opacity_closed_form(means2D, conic_opacity, ranges, point_list, n_contrib, final_t, width, height, g_alpha):
    """dL/dopacity_i of the alpha term written out: sum over the pixels that composited i of g_a T_f G_i / (1 - alpha_i)
    (1 - T_f = 1 - prod (1 - alpha_j); a clamped alpha does not move)."""
    m, co = np.asarray(means2D, np.float64), np.asarray(conic_opacity, np.float64)
    out = np.zeros(m.shape[0])
    for px, py, ids in B._pixel_lists(ranges, point_list, width, height):
        for k in range(int(n_contrib[py, px])):
            g = ids[k]
            dx, dy = m[g, 0] - px, m[g, 1] - py
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            G = np.exp(power)
            raw = co[g, 3] * G
            if power > 0.0 or min(0.99, raw) < 1.0 / 255.0 or raw > 0.99:
                continue
            out[g] += g_alpha[py, px] * final_t[py, px] * G / (1.0 - raw)
    return out


def decisions(means2D, conic_opacity, ranges, point_list, width, height, t_cutoff):
    """Every decision of the blend loop over a scene, as one tuple to compare: per (pixel, record of its list) 0 = not
    reached, 1 = power > 0, 2 = alpha < 1/255, 3 = composited, 4 = composited with alpha clamped to 0.99, 5 = ended the pixel."""
    m, co = np.asarray(means2D, np.float64), np.asarray(conic_opacity, np.float64)
    out = []
    for px, py, ids in B._pixel_lists(ranges, point_list, width, height):
        T, row = 1.0, [0] * len(ids)
        for k, g in enumerate(ids):
            dx, dy = m[g, 0] - px, m[g, 1] - py
            power = -0.5 * (co[g, 0] * dx * dx + co[g, 2] * dy * dy) - co[g, 1] * dx * dy
            if power > 0.0:
                row[k] = 1
                continue
            raw = co[g, 3] * np.exp(power)
            alpha = min(0.99, raw)
            if alpha < 1.0 / 255.0:
                row[k] = 2
                continue
            test = T * (1.0 - alpha)
            if test < t_cutoff:
                row[k] = 5
                break
            row[k] = 4 if raw > 0.99 else 3
            T = test
        out.append(tuple(row))
    return tuple(out)


# ---- the training step (tests/step_autograd_ref.py, tests/step_frames.py, both unchanged) -------------------------------------
def step_reference(raw, cam, case, structure, w, w_a, w_d):
    """The float64 reference of one step with the loss
        (w . color).sum() + (w_a . opacity).sum() + (w_d . depth / opacity.clamp_min(1e-3)).sum()
    on a frame of tests/step_frames.py, made linear in the maps: the quotient's upstream gradients dL/ddepth and dL/dopacity are
    computed in float64 from the reference's own maps (rounded to float32: both sides are handed the same numbers), and the
    gradients are the sum of two step_autograd_ref.gradients() calls — the ordinary one with dL/ddepth as the depth weight,
    and one of colours (1, 0, 0) over a zero background with the weight (dL/dopacity, 0, 0).
    Returns dict: want, want_alpha (gradients keyed by leaf; add them), drop (the pixels left out, step_autograd_ref.pixels_to_drop),
    up_depth, up_opacity (float32 [H,W]), opacity (the reference's map, float64)."""
    import step_autograd_ref as R
    import step_frames as S
    assert S.CASES[case][2] is True and not S.CASES[case][5]
    _, _, ref_depth, aux, drop = S.reference_step(raw, cam, case, structure, w, w_d)
    opacity = 1.0 - aux["finalT"]
    clamp = np.maximum(opacity, 1e-3)
    up_depth = (w_d / clamp).astype(np.float32)
    up_opacity = (w_a + np.where(opacity > 1e-3, -w_d * ref_depth / (clamp * clamp), 0.0)).astype(np.float32)
    want = R.gradients(R.leaves(raw, cam), structure, cam, w, up_depth, drop, **S.forward_options(case))[0]
    raw_a = dict(raw, colors=np.tile(np.array([1.0, 0.0, 0.0], np.float32), (S.N, 1)))
    w3 = np.zeros((3, S.H, S.W), np.float32)
    w3[0] = up_opacity
    opts = dict(S.forward_options(case), background=(0.0, 0.0, 0.0), depth=False)
    want_alpha = R.gradients(R.leaves(raw_a, cam, colors=True), structure, cam, w3, np.zeros((S.H, S.W), np.float32), drop, **opts)[0]
    return dict(want=want, want_alpha=want_alpha, drop=drop, up_depth=up_depth, up_opacity=up_opacity, opacity=opacity)


def step_quotient_autograd(raw, cam, case, structure, w, w_a, w_d, drop):
    """The same step without the linearisation: the restated forward run twice over the same leaves (the scene's colours,
    and colours (1, 0, 0) over a zero background, whose first channel is the opacity), the quotient loss as written, and
    torch.autograd. Returns the gradients keyed by leaf (float64 numpy)."""
    import torch
    import step_autograd_ref as R
    import step_frames as S
    leaf = R.leaves(raw, cam)
    color, dmap, _ = R.forward(leaf, structure, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, **S.forward_options(case))
    ones = torch.zeros((S.N, 3), dtype=R.F64)
    ones[:, 0] = 1.0
    opts = dict(S.forward_options(case), background=(0.0, 0.0, 0.0), depth=False)
    opacity = R.forward(dict(leaf, colors=ones), structure, cam.tan_fovx, cam.tan_fovy, cam.width, cam.height, **opts)[0][0]
    keep = torch.from_numpy(~drop)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(R.F64) * keep
    loss = (t(w) * color).sum() + (t(w_a) * opacity).sum() + (t(w_d) * dmap / opacity.clamp_min(1e-3)).sum()
    got = torch.autograd.grad(loss, list(leaf.values()), allow_unused=True)
    return {k: (g.numpy() if g is not None else np.zeros(tuple(v.shape))) for (k, v), g in zip(leaf.items(), got)}
