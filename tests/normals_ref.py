"""References of the two operators of the normal-consistency loss (include/gsrast_amd_normals.h), shared by
tests/test_normals_cpu.py and tests/test_gpu_normals.py with the seeded cases both files use.

Forward: float32 numpy restatements written from the header, operation by operation (numpy's float32 +, -, *, / and sqrt are
IEEE; nothing is fused), with the decisions they took (the axis, the flip, the validity) beside the values.
Backward: torch autograd over float64 copies of the float32 inputs, fed those float32 decisions. For the depth normal the four
neighbour depths of a pixel are read from four separate leaves, so that the gradient of each leaf is one of the four terms the
header's gather adds: up, left, right, down."""
import functools

import numpy as np
import torch

F = np.float32
PROFILES = ("gscuda", "inria")


# ---- the per-Gaussian normal ------------------------------------------------------------------------------------------------------
def _column_f32(q, a, semantics):
    """Column a[i] of the profile's R for every row, float32 [N,3], as the header writes the entries."""
    q = np.asarray(q, F)
    with np.errstate(all="ignore"):
        if semantics == "inria":
            r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
            one, two = F(1.0), F(2.0)
            cols = [np.stack([one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)], 1),
                    np.stack([two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)], 1),
                    np.stack([two * (x * z + r * y), two * (y * z - r * x), one - two * (x * x + y * y)], 1)]
        else:
            dq = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + (q[:, 2] * q[:, 2] + q[:, 3] * q[:, 3])
            inv = F(1.0) / np.sqrt(dq)
            x, y, z, w = q[:, 0] * inv, q[:, 1] * inv, q[:, 2] * inv, q[:, 3] * inv
            D = lambda u: (2.0 * u.astype(np.float64) - 1.0).astype(F)
            E = lambda u: (2.0 * u.astype(np.float64)).astype(F)
            cols = [np.stack([D(x * x + y * y), E(y * z + x * w), E(y * w - x * z)], 1),
                    np.stack([E(y * z - x * w), D(x * x + z * z), E(z * w + x * y)], 1),
                    np.stack([E(y * w + x * z), E(z * w - x * y), D(x * x + w * w)], 1)]
    return np.stack(cols, 1)[np.arange(len(q)), a].astype(F)


def shortest_axis(scales):
    s = np.asarray(scales, F)
    a = np.zeros(len(s), np.int64)
    with np.errstate(invalid="ignore"):
        a = np.where(s[:, 1] < s[np.arange(len(s)), a], 1, a)
        a = np.where(s[:, 2] < s[np.arange(len(s)), a], 2, a)
    return a


def gaussian_normals_f32(means3D, scales, rotations, view, semantics):
    """(normals [N,3] float32, decisions): the header's gsr_gaussian_normals_forward. decisions: axis [N], flipped [N], valid [N]."""
    m, v = np.asarray(means3D, F), np.asarray(view, F).reshape(16)
    a = shortest_axis(scales)
    nw = _column_f32(rotations, a, semantics)
    with np.errstate(all="ignore"):
        if semantics == "inria":
            t = [((v[r] * m[:, 0] + v[4 + r] * m[:, 1]) + v[8 + r] * m[:, 2]) + v[12 + r] for r in range(3)]
        else:
            t = [(v[r] * m[:, 0] + v[4 + r] * m[:, 1]) + (v[8 + r] * m[:, 2] + v[12 + r] * F(1.0)) for r in range(3)]
        nv = np.stack([(v[r] * nw[:, 0] + v[4 + r] * nw[:, 1]) + v[8 + r] * nw[:, 2] for r in range(3)], 1).astype(F)
        d = (nv[:, 0] * t[0] + nv[:, 1] * t[1]) + nv[:, 2] * t[2]
        flipped = d > 0
        nv = np.where(flipped[:, None], -nv, nv)
        l = np.sqrt((nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1]) + nv[:, 2] * nv[:, 2])
        valid = np.isfinite(l) & (l != 0)
        out = np.where(valid[:, None], nv / l[:, None], F(0.0)).astype(F)
    return out, {"axis": a, "flipped": flipped, "valid": valid}


def gaussian_normals64(rotations, view, decisions, semantics):
    """The same function of float64 torch tensors with the decisions given: [N,3]; rows that are not valid are 0 (no gradient)."""
    q, v = rotations, view.reshape(16)
    if semantics == "inria":
        r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        cols = [torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1),
                torch.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1),
                torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], 1)]
    else:
        qn = q / q.norm(dim=1, keepdim=True)
        x, y, z, w = qn[:, 0], qn[:, 1], qn[:, 2], qn[:, 3]
        cols = [torch.stack([2 * (x * x + y * y) - 1, 2 * (y * z + x * w), 2 * (y * w - x * z)], 1),
                torch.stack([2 * (y * z - x * w), 2 * (x * x + z * z) - 1, 2 * (z * w + x * y)], 1),
                torch.stack([2 * (y * w + x * z), 2 * (z * w - x * y), 2 * (x * x + w * w) - 1], 1)]
    n = len(q)
    nw = torch.stack(cols, 1)[torch.arange(n), torch.from_numpy(np.asarray(decisions["axis"]))]
    Wm = torch.stack([torch.stack([v[4 * c + r] for c in range(3)]) for r in range(3)])          # W[r][c] = V(r, c)
    sigma = torch.from_numpy(np.where(decisions["flipped"], -1.0, 1.0)).to(nw.dtype)
    nv = (nw @ Wm.T) * sigma[:, None]
    valid = torch.from_numpy(np.asarray(decisions["valid"]))
    safe = torch.where(valid[:, None], nv, torch.ones_like(nv))
    return torch.where(valid[:, None], safe / safe.norm(dim=1, keepdim=True), torch.zeros_like(nv))


def gaussian_gradients64(rotations, view, g, decisions, semantics):
    """dL_drotations [N,4] float64 of sum(g * normals) by autograd over float64 copies; rows that are not valid get 0."""
    valid = np.asarray(decisions["valid"])
    q = torch.from_numpy(np.where(valid[:, None], np.asarray(rotations, np.float64), 1.0)).requires_grad_(True)
    out = gaussian_normals64(q, torch.from_numpy(np.asarray(view, np.float64)), decisions, semantics)
    (out * torch.from_numpy(np.where(valid[:, None], np.asarray(g, np.float64), 0.0))).sum().backward()
    return q.grad.numpy() * valid[:, None]


def random_view(seed, mirrored=False):
    """16 floats, column-major: a seeded rotation and a translation that puts the origin 5 units in front (z > 0). mirrored: row 2
    of the rotation negated, a determinant of -1 as the reference's caller hands over."""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    if mirrored:
        Rm[2] *= -1.0
    V = np.eye(4)
    V[:3, :3] = Rm
    V[:3, 3] = (0.3, -0.2, 5.0)
    return np.ascontiguousarray(V.T.reshape(-1).astype(F))          # column-major: V[4 c + r]


@functools.lru_cache(maxsize=None)
def gaussian_case(n, seed=0, edges=True):
    """(means3D [n,4], scales [n,4], rotations [n,4]) float32, read-only: seeded rows around the origin (random_view sees them some
    5 units ahead; a tenth of them behind it), quaternions of lengths 0.5 .. 2; with edges, the first rows hold the edge values:
    ties in every pair and in all three scales, zeros, 1e9, a NaN scale, a zero quaternion, a NaN quaternion."""
    rng = np.random.default_rng(1000 * seed + n)
    means = np.ones((n, 4), F)
    means[:, :3] = rng.normal(0.0, 1.5, (n, 3))
    behind = rng.uniform(size=n) < 0.1
    means[behind, :3] *= F(8.0)
    scales = np.exp(rng.normal(-2.0, 1.0, (n, 4))).astype(F)
    scales[:, 3] = F(np.e)
    q = rng.normal(size=(n, 4))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (n, 1))).astype(F)
    if edges:
        rows = [((0.1, 0.1, 0.5), None), ((0.5, 0.1, 0.1), None), ((0.1, 0.5, 0.1), None), ((0.2, 0.2, 0.2), None),
                ((0.0, 0.0, 1.0), None), ((1.0, 0.0, 0.0), None), ((1e9, 1e9, 1.0), None), ((1.0, 1e9, 1e9), None),
                ((np.nan, 0.3, 0.2), None), ((0.3, np.nan, 0.2), None), ((0.3, 0.2, np.nan), None),
                (None, (0.0, 0.0, 0.0, 0.0)), (None, (np.nan, 0.1, 0.2, 0.3)), (None, (3.0, 0.0, 0.0, 0.0)), (None, (1e-30, 0.0, 0.0, 0.0))]
        for i, (s, quat) in enumerate(rows[:n]):
            if s is not None:
                scales[i, :3] = s
            if quat is not None:
                q[i] = quat
    for a in (means, scales, q):
        a.setflags(write=False)
    return means, scales, q


def seed_gradient(shape, seed=5):
    return np.random.default_rng(seed).normal(size=shape).astype(F)


# ---- the normal of a depth surface --------------------------------------------------------------------------------------------------
def ndc(i, size, semantics, dtype=F):
    """ndc_x / ndc_y of the header for integer coordinates i (an array), in `dtype` arithmetic."""
    i, size = np.asarray(i).astype(dtype), dtype(F(size))
    two, one = dtype(2.0), dtype(1.0)
    return ((two * i + one) / size - one) if semantics == "inria" else ((two * i) / size - one)


def depth_normals_f32(depth, tan_fov, semantics):
    """(normals [3,H,W] float32, decisions): the header's gsr_depth_normals_forward. decisions: interior, finite (the four
    neighbours are finite and > 0), flipped, valid, all bool [H,W]."""
    D = np.asarray(depth, F)
    H, W = D.shape
    out = np.zeros((3, H, W), F)
    dec = {k: np.zeros((H, W), bool) for k in ("interior", "finite", "flipped", "valid")}
    if H < 3 or W < 3:
        return out, dec
    tx, ty = F(tan_fov[0]), F(tan_fov[1])
    xs, ys = np.arange(1, W - 1), np.arange(1, H - 1)
    rx, rxl, rxr = (ndc(xs + k, W, semantics) * tx for k in (0, -1, 1))
    ry, ryu, ryd = (ndc(ys + k, H, semantics) * ty for k in (0, -1, 1))
    rx, rxl, rxr = rx[None, :], rxl[None, :], rxr[None, :]
    ry, ryu, ryd = ry[:, None], ryu[:, None], ryd[:, None]
    du, dd, dl, dr = D[:-2, 1:-1], D[2:, 1:-1], D[1:-1, :-2], D[1:-1, 2:]
    with np.errstate(all="ignore"):
        ok = lambda d: np.isfinite(d) & (d > 0)
        finite = ok(du) & ok(dd) & ok(dl) & ok(dr)
        dvx, dvy, dvz = rx * dd - rx * du, ryd * dd - ryu * du, dd - du
        dhx, dhy, dhz = rxr * dr - rxl * dl, ry * dr - ry * dl, dr - dl
        cx, cy, cz = dvy * dhz - dvz * dhy, dvz * dhx - dvx * dhz, dvx * dhy - dvy * dhx
        flipped = (cx * rx + cy * ry) + cz > 0
        cx, cy, cz = (np.where(flipped, -c, c) for c in (cx, cy, cz))
        l = np.sqrt((cx * cx + cy * cy) + cz * cz)
        valid = finite & np.isfinite(l) & (l != 0)
        for k, c in enumerate((cx, cy, cz)):
            out[k, 1:-1, 1:-1] = np.where(valid, c / l, F(0.0))
    dec["interior"][1:-1, 1:-1] = True
    dec["finite"][1:-1, 1:-1] = finite
    dec["flipped"][1:-1, 1:-1] = flipped & valid
    dec["valid"][1:-1, 1:-1] = valid
    return out, dec


def depth_normals64(Du, Dl, Dr, Dd, tan_fov, semantics, decisions):
    """The same function of float64 torch images with the decisions given: the up / left / right / down neighbour of a pixel is
    read from Du / Dl / Dr / Dd (the same image four times, or four leaves of it). [3,H,W]; 0 where not valid."""
    H, W = Du.shape
    out = torch.zeros((3, H, W), dtype=Du.dtype)                              # (float64; tests/step_autograd_ref.py also runs it in float32)
    if H < 3 or W < 3:
        return out
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64)).to(Du.dtype)
    tx, ty = np.float64(F(tan_fov[0])), np.float64(F(tan_fov[1]))
    xs, ys = np.arange(1, W - 1), np.arange(1, H - 1)
    rx, rxl, rxr = (t(ndc(xs + k, W, semantics, np.float64) * tx)[None, :] for k in (0, -1, 1))
    ry, ryu, ryd = (t(ndc(ys + k, H, semantics, np.float64) * ty)[:, None] for k in (0, -1, 1))
    valid = torch.from_numpy(decisions["valid"][1:-1, 1:-1])
    pick = lambda img: torch.where(valid, img, torch.ones_like(img))          # (holes: NaN and inf stay out of the graph)
    du, dd, dl, dr = pick(Du[:-2, 1:-1]), pick(Dd[2:, 1:-1]), pick(Dl[1:-1, :-2]), pick(Dr[1:-1, 2:])
    dvx, dvy, dvz = rx * dd - rx * du, ryd * dd - ryu * du, dd - du
    dhx, dhy, dhz = rxr * dr - rxl * dl, ry * dr - ry * dl, dr - dl
    c = torch.stack([dvy * dhz - dvz * dhy, dvz * dhx - dvx * dhz, dvx * dhy - dvy * dhx])
    c = c * t(np.where(decisions["flipped"][1:-1, 1:-1], -1.0, 1.0))
    safe = torch.where(valid, c, torch.ones_like(c))
    out[:, 1:-1, 1:-1] = torch.where(valid, safe / safe.norm(dim=0, keepdim=True), torch.zeros_like(c))
    return out


def depth_gradients64(depth, g, tan_fov, semantics, decisions=None):
    """(dL_ddepth [H,W], terms [4,H,W]) float64 of sum(g * normals): terms[0..3] are the shares of the pixel's up, left, right and
    down neighbour's normal — the pixel is that neighbour's down, right, left, up depth — and dL_ddepth is ((up + left) + right) +
    down."""
    if decisions is None:
        decisions = depth_normals_f32(depth, tan_fov, semantics)[1]
    clean = np.where(np.isfinite(np.asarray(depth, np.float64)), np.asarray(depth, np.float64), 1.0)
    if min(clean.shape) < 3:                                                                  # (no interior pixel: no graph)
        return np.zeros(clean.shape), np.zeros((4,) + clean.shape)
    leaves = [torch.from_numpy(clean.copy()).requires_grad_(True) for _ in range(4)]          # read as Du, Dl, Dr, Dd
    out = depth_normals64(*leaves, tan_fov, semantics, decisions)
    (out * torch.from_numpy(np.asarray(g, np.float64))).sum().backward()
    grad = [np.zeros(clean.shape) if l.grad is None else l.grad.numpy() for l in leaves]
    terms = np.stack([grad[3], grad[2], grad[1], grad[0]])
    return ((terms[0] + terms[1]) + terms[2]) + terms[3], terms


TAN_FOV = (0.7, 0.45)
HOLES = (0.0, -1.0, np.inf, -np.inf, np.nan)


@functools.lru_cache(maxsize=None)
def depth_case(h, w, seed=0, holes=0.04):
    """A seeded depth image [h,w] float32, read-only: a smooth surface between 2 and 6 with a step edge and fine noise, and a share
    `holes` of its pixels replaced by 0, -1, +-inf and NaN in turn. (No image of positive depths flips a normal: with the pixel's
    ray r the mean of its neighbours' rays, c . r = -(Dd + Du)(Dr + Dl) dx dy < 0 in exact arithmetic; the header's test guards
    the rounding, and the seeded cases cannot reach it.)"""
    rng = np.random.default_rng(7919 * seed + 1000 * h + w)
    ys, xs = np.mgrid[0:h, 0:w]
    d = 4.0 + 0.8 * np.sin(0.31 * xs + rng.uniform(0, 6)) + 0.6 * np.cos(0.23 * ys + rng.uniform(0, 6)) + 0.02 * rng.normal(size=(h, w))
    d = np.where(xs + 2 * ys > 0.9 * (w + 2 * h), d + 1.0, d).astype(F)
    where = np.nonzero(rng.uniform(size=(h, w)) < holes)
    d[where] = np.array(HOLES, F)[np.arange(len(where[0])) % len(HOLES)]
    d.setflags(write=False)
    return d


def plane_depth(h, w, normal, offset, tan_fov, semantics):
    """The depth image (float64) of the plane normal . P = offset seen along the header's rays: D = offset / (normal . (rx, ry, 1))."""
    rx = ndc(np.arange(w), w, semantics, np.float64) * np.float64(F(tan_fov[0]))
    ry = ndc(np.arange(h), h, semantics, np.float64) * np.float64(F(tan_fov[1]))
    return offset / (normal[0] * rx[None, :] + normal[1] * ry[:, None] + normal[2])


def ulp32(x):
    x = np.abs(np.asarray(x, np.float64)).astype(F)
    return (np.nextafter(x, F(np.inf)) - x).astype(np.float64)
