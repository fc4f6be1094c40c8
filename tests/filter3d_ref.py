"""References of the 3D smoothing filter (include/gsrast_amd_filter3d.h), shared by tests/test_filter3d_cpu.py and
tests/test_gpu_filter3d.py:

  observe_f32 / finalize_f32 / forward_f32   numpy float32 restatements of the header, operation for operation: what the
                                             kernels are compared with bit for bit
  smoothing64 / gradients64                  the smoothing as a float64 torch-autograd function, fed the float32 IDENTITY decision
  upstream_filter64                          a float64 transcription of upstream's compute_3D_filter, written the upstream
                                             way (masks, xyz @ R + T, the 100000 cap and the flag array)
"""
import numpy as np
import torch

F = np.float32
K_BITS = 0x3EE4F92E
K = np.array([K_BITS], np.uint32).view(np.float32)[0]
INF = F(np.inf)


def observe_f32(positions, records, min_depth=None, detail=False):
    """min_depth [N] after the cameras `records` [C,20]; detail=True: also per camera the masks (valid, depth_ok, in_x_lo,
    in_x_hi, in_y_lo, in_y_hi, px, py, t2) as a list of dicts."""
    p = np.ascontiguousarray(positions, F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    md = np.full(p.shape[0], INF, F) if min_depth is None else np.array(min_depth, F)
    out = []
    with np.errstate(all="ignore"):
        for c in np.ascontiguousarray(records, F).reshape(-1, 20):
            t = [((c[4 * r] * x + c[4 * r + 1] * y) + c[4 * r + 2] * z) + c[4 * r + 3] for r in range(3)]
            zc = np.where(t[2] < F(0.001), F(0.001), t[2]).astype(F)           # glm max(t_2, 0.001f)
            px = (t[0] / zc) * c[12] + c[14]
            py = (t[1] / zc) * c[13] + c[15]
            m = {"depth_ok": t[2] > F(0.2), "in_x_lo": px >= c[16], "in_x_hi": px <= c[17], "in_y_lo": py >= c[18], "in_y_hi": py <= c[19]}
            valid = m["depth_ok"] & m["in_x_lo"] & m["in_x_hi"] & m["in_y_lo"] & m["in_y_hi"]
            md = np.where(valid & (t[2] < md), t[2], md).astype(F)               # glm min(min_depth, t_2)
            if detail:
                m.update(valid=valid, px=px, py=py, t2=t[2])
                out.append(m)
    return (md, out) if detail else md


def finalize_f32(min_depth, max_focal):
    md = np.asarray(min_depth, F)
    seen = md < INF
    d_max = md[seen].max() if seen.any() else F(0.0)
    d = np.where(seen, md, d_max).astype(F)
    return ((d / F(max_focal)) * K).astype(F)


def forward_f32(scales, opacities, filt):
    """dict: scales_out [N,4], opacities_out [N], coef [N], identity bool[N]."""
    s4 = np.ascontiguousarray(scales, F)
    o, f = np.asarray(opacities, F), np.asarray(filt, F)
    with np.errstate(all="ignore"):
        f2 = f * f
        identity = ~(f2 > F(0.0))
        q = s4[:, :3] * s4[:, :3]
        a = q + f2[:, None]
        sp = np.sqrt(a).astype(F)
        r = (q / a).astype(F)
        coef = np.sqrt((r[:, 0] * r[:, 1]) * r[:, 2]).astype(F)
        o_out = np.where(identity, o, o * coef).astype(F)
    s_out = s4.copy()
    s_out[:, :3] = np.where(identity[:, None], s4[:, :3], sp)
    # (np.where keeps the bits of whichever side it takes, a NaN's payload included)
    o_out = np.where(identity, o.view(np.uint32), o_out.view(np.uint32)).view(F)
    return {"scales_out": s_out, "opacities_out": o_out, "coef": coef, "identity": identity}


def det_ratio_coef_f32(scales, filt):
    """Upstream's coefficient the upstream way, in float32: sqrt(det1 / det2) of the two products."""
    s, f = np.asarray(scales, F)[:, :3], np.asarray(filt, F)
    with np.errstate(all="ignore"):
        q = s * s
        det1 = q[:, 0] * q[:, 1] * q[:, 2]
        a = q + (f * f)[:, None]
        det2 = a[:, 0] * a[:, 1] * a[:, 2]
        return np.sqrt(det1 / det2).astype(F)


def smoothing64(scales, opacities, filt, identity):
    """float64 tensors scales [N,3], opacities [N], filt [N]; identity bool [N] (the float32 forward's decision).
    Returns (scales' [N,3], opacities' [N]). |s| / sqrt(a): the header's u_k, whose derivative at 0 is taken as sign(0) = 0."""
    f2 = (filt * filt)[:, None]
    a = scales * scales + f2
    sp = torch.sqrt(a)
    u = torch.abs(scales) / sp
    coef = u[:, 0] * u[:, 1] * u[:, 2]
    ident = torch.as_tensor(identity)
    return torch.where(ident[:, None], scales, sp), torch.where(ident, opacities, opacities * coef)


def gradients64(scales, opacities, filt, g_scales, g_opacities, identity=None):
    """{"scales": [N,3], "opacities": [N]} float64: dL/ds and dL/do of L = sum(g_s . s') + sum(g_o o'), by autograd."""
    if identity is None:
        identity = forward_f32(scales, opacities, filt)["identity"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64))
    s = t(np.asarray(scales)[:, :3]).requires_grad_(True)
    o = t(opacities).requires_grad_(True)
    sp, op = smoothing64(s, o, t(filt), identity)
    loss = (sp * t(np.asarray(g_scales)[:, :3])).sum() + (op * t(g_opacities)).sum()
    gs, go = torch.autograd.grad(loss, (s, o))
    return {"scales": gs.numpy(), "opacities": go.numpy()}


def upstream_cameras(cameras):
    """Camera objects -> what upstream's loop reads of a camera: (R [3,3], T [3], focal_x, focal_y, width, height) in float64,
    with upstream's convention xyz_cam = xyz @ R + T (R is the transposed world-to-camera rotation)."""
    out = []
    for cam in cameras:
        V = np.asarray(cam.view, np.float64).reshape(4, 4).T          # V[r][c]; row 2 already points forward
        out.append((V[:3, :3].T.copy(), V[:3, 3].copy(), cam.width / (2.0 * cam.tan_fovx), cam.height / (2.0 * cam.tan_fovy),
                    cam.width, cam.height))
    return out


def upstream_filter64(xyz, cameras, detail=False):
    """Upstream's compute_3D_filter in float64 torch, the upstream way. Returns filter_3D [N] (and, with detail, the distance
    array, the valid_points flags and per camera (x, y, z_unclamped))."""
    xyz = torch.from_numpy(np.ascontiguousarray(np.asarray(xyz)[:, :3], np.float64))
    distance = torch.ones((xyz.shape[0]), dtype=torch.float64) * 100000.0
    valid_points = torch.zeros((xyz.shape[0]), dtype=torch.bool)
    focal_length = 0.0
    per_camera = []
    for R, T, focal_x, focal_y, width, height in upstream_cameras(cameras):
        R, T = torch.from_numpy(R), torch.from_numpy(T)
        xyz_cam = xyz @ R + T[None, :]
        valid_depth = xyz_cam[:, 2] > 0.2
        x, y, z = xyz_cam[:, 0], xyz_cam[:, 1], xyz_cam[:, 2]
        z_raw = z
        z = torch.clamp(z, min=0.001)
        x = x / z * focal_x + width / 2.0
        y = y / z * focal_y + height / 2.0
        in_screen = torch.logical_and(torch.logical_and(x >= -0.15 * width, x <= width * 1.15),
                                      torch.logical_and(y >= -0.15 * height, y <= 1.15 * height))
        valid = torch.logical_and(valid_depth, in_screen)
        distance[valid] = torch.min(distance[valid], z[valid])
        valid_points = torch.logical_or(valid_points, valid)
        if focal_length < focal_x:
            focal_length = focal_x
        per_camera.append((x.numpy(), y.numpy(), z_raw.numpy()))
    distance[~valid_points] = distance[valid_points].max()
    filter_3D = distance / focal_length * (0.2 ** 0.5)
    if detail:
        return filter_3D.numpy(), distance.numpy(), valid_points.numpy(), per_camera
    return filter_3D.numpy()


def exact_camera(width=640, height=480, focal=512.0):
    """An identity-rotation camera at the origin looking down +z (after the negation of row 2: t = (x, y, z)) whose record is
    exact: focal 512, 640 x 480, so that the four bounds are the integers -96, 736, -72, 552 and, at t_2 a power of two, px, py
    and t_2 are computed without rounding."""
    from gsrast_amd.camera import Camera
    view = np.eye(4, dtype=F)
    return Camera(view=view.T.reshape(16).copy(), proj=view.T.reshape(16).copy(), cam_pos=np.zeros(3, F),
                  tan_fovx=width / (2.0 * focal), tan_fovy=height / (2.0 * focal), width=width, height=height)


def orbit_cameras(count, width=96, height=64, radius=5.0, seed=0, arc=None):
    """`count` first_person_camera poses around the origin, each looking roughly at it; arc: the angle they are spread over
    (radians, from the default pose's side; default: the full circle)."""
    import math
    from gsrast_amd.camera import first_person_camera
    rng = np.random.default_rng(seed)
    cams = []
    for k in range(count):
        ang = (2.0 * math.pi if arc is None else arc) * k / max(count, 1) + float(rng.uniform(-0.1, 0.1))
        r = radius * float(rng.uniform(0.6, 1.4))
        pos = (-r * math.sin(ang), float(rng.uniform(-0.5, 0.5)), -r * math.cos(ang))
        cams.append(first_person_camera(pos, ang + float(rng.uniform(-0.2, 0.2)), float(rng.uniform(-0.1, 0.1)), math.radians(45.0),
                                        0.05, 50.0, width, height))
    return cams


def seeded_points(n, seed=0, spread=4.0, stride=3):
    rng = np.random.default_rng(seed)
    p = np.ones((n, stride), F)
    p[:, :3] = rng.uniform(-spread, spread, (n, 3)).astype(F)
    return p


def boundary_guard(xyz, cameras, rel=1e-4):
    """bool: no (point, camera) pair lies within a relative `rel` of any of the five boundaries (float64, the upstream way)."""
    _, _, _, per_camera = upstream_filter64(xyz, cameras, detail=True)
    for (x, y, z), cam in zip(per_camera, cameras):
        w, h = cam.width, cam.height
        near = np.abs(z - 0.2) <= rel * 0.2
        for v, bound, size in ((x, -0.15 * w, w), (x, 1.15 * w, w), (y, -0.15 * h, h), (y, 1.15 * h, h)):
            near |= (np.abs(v - bound) <= rel * size) & (z > 0.1)
        if near.any():
            return False
    return True
