"""Float64 reference of the camera gradients (gsr_camera_backward): dL / d(view_matrix, proj_matrix, cam_pos) from the
per-Gaussian gradients of gsr_backward. Written in torch so that the same code runs on the host (float64 CPU tensors, the
CPU tests) and on the device (the full-size GPU test). tests/test_camera_grad_cpu.py pins it against central differences
of the float64 per-Gaussian forward functions of oracle/backward_np.py.

Layout of a camera gradient: 35 floats, view (16) | proj (16) | cam_pos (3), the matrices column-major as gsr_forward
takes them (entry (row r, column c) at 4 c + r)."""
from __future__ import annotations

import numpy as np
import torch

from oracle import backward_np as B

F64, F32 = torch.float64, torch.float32


def _t(x, dev, dtype):
    if isinstance(x, torch.Tensor):
        return x.to(device=dev, dtype=dtype)
    return torch.as_tensor(np.ascontiguousarray(x), device=dev).to(dtype)


def focal_lengths(width, height, tan_fovx, tan_fovy, inria, f32=True):
    """The chain's focal lengths: gscuda one, H / (2 tan_fovy), for both axes; upstream W / (2 tan_fovx), H / (2 tan_fovy).
    f32: computed in float32 as the library computes them."""
    if f32:
        fy = float(np.float32(height) / (np.float32(2.0) * np.float32(tan_fovy)))
        fx = float(np.float32(width) / (np.float32(2.0) * np.float32(tan_fovx))) if inria else fy
    else:
        fy = height / (2.0 * tan_fovy)
        fx = width / (2.0 * tan_fovx) if inria else fy
    return fx, fy


def _sh_grad_basis(d, deg):
    """dB_k / d dir [n, 16, 3] at the unit directions d [n, 3] (zeros beyond `deg`; oracle: sh_basis)."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    G = torch.zeros(d.shape[0], 16, 3, dtype=d.dtype, device=d.device)
    C1, C2, C3 = B.SH_C1, B.SH_C2, B.SH_C3
    if deg > 0:
        G[:, 1, 1], G[:, 2, 2], G[:, 3, 0] = -C1, C1, -C1
    if deg > 1:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        G[:, 4, 0], G[:, 4, 1] = C2[0] * y, C2[0] * x
        G[:, 5, 1], G[:, 5, 2] = C2[1] * z, C2[1] * y
        G[:, 6, 0], G[:, 6, 1], G[:, 6, 2] = -2 * C2[2] * x, -2 * C2[2] * y, 4 * C2[2] * z
        G[:, 7, 0], G[:, 7, 2] = C2[3] * z, C2[3] * x
        G[:, 8, 0], G[:, 8, 1] = 2 * C2[4] * x, -2 * C2[4] * y
        if deg > 2:
            G[:, 9, 0], G[:, 9, 1] = C3[0] * 6 * xy, C3[0] * (3 * xx - 3 * yy)
            G[:, 10, 0], G[:, 10, 1], G[:, 10, 2] = C3[1] * yz, C3[1] * xz, C3[1] * xy
            G[:, 11, 0], G[:, 11, 1], G[:, 11, 2] = C3[2] * -2 * xy, C3[2] * (4 * zz - xx - 3 * yy), C3[2] * 8 * yz
            G[:, 12, 0], G[:, 12, 1], G[:, 12, 2] = C3[3] * -6 * xz, C3[3] * -6 * yz, C3[3] * (6 * zz - 3 * xx - 3 * yy)
            G[:, 13, 0], G[:, 13, 1], G[:, 13, 2] = C3[4] * (4 * zz - 3 * xx - yy), C3[4] * -2 * xy, C3[4] * 8 * xz
            G[:, 14, 0], G[:, 14, 1], G[:, 14, 2] = C3[5] * 2 * xz, C3[5] * -2 * yz, C3[5] * (xx - yy)
            G[:, 15, 0], G[:, 15, 1] = C3[6] * (3 * xx - 3 * yy), C3[6] * -6 * xy
    return G


def camera_terms(means3D, view, proj, cam_pos, tan_fovx, tan_fovy, width, height, radii, cov3D, dL_dmean2D, dL_dcov2D,
                 dL_ddepths=None, inverse=False, inria=False, shs=None, sh_degree=0, dL_dcolors=None, clamped=None,
                 f32_decisions=True, device="cpu"):
    """(vis, T): the indices of the visible Gaussians (radii > 0) and their camera terms T [len(vis), 35] in float64.
    means3D [N,4]; view / proj 16 floats; cov3D [N,6]; dL_dmean2D [N,2]; dL_dcov2D [N,>=3] (m00, m01, m11); dL_ddepths [N]
    or None; upstream colour: shs [N,48] ([16][3]), dL_dcolors [N,3], clamped [N,3] (shs None: no colour term).
    f32_decisions: t and the clamp decisions of t.x / t.z, t.y / t.z in float32 in the library's operation order, the
    focal lengths in float32 (what the kernel does); else everything in float64 (what the finite differences see)."""
    dev = torch.device(device)
    vis = torch.nonzero(_t(radii, dev, torch.int64) > 0).flatten()
    m32 = _t(means3D, dev, F32)[vis]
    v32, p32 = _t(view, dev, F32).reshape(16), _t(proj, dev, F32).reshape(16)
    v, pm = v32.to(F64), p32.to(F64)
    x, y, z, mw4 = (m32[:, k].to(F64) for k in range(4))
    if f32_decisions:
        X, Y, Z = m32[:, 0], m32[:, 1], m32[:, 2]
        one = torch.ones((), dtype=F32, device=dev)
        txf = (v32[0] * X + v32[4] * Y) + (v32[8] * Z + v32[12] * one)
        tyf = (v32[1] * X + v32[5] * Y) + (v32[9] * Z + v32[13] * one)
        tzf = (v32[2] * X + v32[6] * Y) + (v32[10] * Z + v32[14] * one)
        limx = torch.tensor(np.float32(1.3) * np.float32(tan_fovx), dtype=F32, device=dev)
        limy = torch.tensor(np.float32(1.3) * np.float32(tan_fovy), dtype=F32, device=dev)
        rx, ry = txf / tzf, tyf / tzf
        cxf, cyf = torch.minimum(limx, torch.maximum(-limx, rx)), torch.minimum(limy, torch.maximum(-limy, ry))
        clx, cly = rx != cxf, ry != cyf
        tz, cx, cy = tzf.to(F64), cxf.to(F64), cyf.to(F64)
    else:
        t0 = v[0] * x + v[4] * y + v[8] * z + v[12]
        t1 = v[1] * x + v[5] * y + v[9] * z + v[13]
        tz = v[2] * x + v[6] * y + v[10] * z + v[14]
        limx, limy = 1.3 * float(tan_fovx), 1.3 * float(tan_fovy)
        rx, ry = t0 / tz, t1 / tz
        cx, cy = rx.clamp(-limx, limx), ry.clamp(-limy, limy)
        clx, cly = rx != cx, ry != cy
    tx, ty = cx * tz, cy * tz
    fx, fy = focal_lengths(width, height, tan_fovx, tan_fovy, inria, f32_decisions)
    nv = vis.numel()
    zero = torch.zeros(nv, dtype=F64, device=dev)
    J = torch.stack([torch.stack([fx / tz, zero, -fx * tx / (tz * tz)], 1),
                     torch.stack([zero, fy / tz, -fy * ty / (tz * tz)], 1)], 1)               # [nv, 2, 3]
    W = v.reshape(4, 4).T[:3, :3]                                                           # W[r, c] = V[4 c + r]
    c3 = _t(cov3D, dev, F64)[vis]
    S = torch.stack([torch.stack([c3[:, 0], c3[:, 1], c3[:, 2]], 1), torch.stack([c3[:, 1], c3[:, 3], c3[:, 4]], 1),
                     torch.stack([c3[:, 2], c3[:, 4], c3[:, 5]], 1)], 1)
    gc = _t(dL_dcov2D, dev, F64)[vis]
    gM = torch.stack([torch.stack([gc[:, 0], gc[:, 1]], 1), torch.stack([gc[:, 1], gc[:, 2]], 1)], 1)
    P = J @ W
    gP = 2.0 * gM @ P @ S                        # dL/dP of tr(gM P S P^T)
    dW = J.transpose(1, 2) @ gP                  # dL/dW, W = upper 3 x 3 of V
    gJ = gP @ W.T                                # dL/dJ
    g_tx = -gJ[:, 0, 2] * fx / (tz * tz)
    g_ty = -gJ[:, 1, 2] * fy / (tz * tz)
    g_tz = (-gJ[:, 0, 0] * fx - gJ[:, 1, 1] * fy) / (tz * tz) + (gJ[:, 0, 2] * fx * tx + gJ[:, 1, 2] * fy * ty) * (2.0 / tz ** 3)
    gt = torch.stack([torch.where(clx, zero, g_tx), torch.where(cly, zero, g_ty),
                      g_tz + torch.where(clx, g_tx * cx, zero) + torch.where(cly, g_ty * cy, zero)], 1)
    if dL_ddepths is not None:
        gd = _t(dL_ddepths, dev, F64)[vis]
        gt[:, 2] += -gd / (tz * tz) if inverse else gd
    T = torch.zeros(nv, 35, dtype=F64, device=dev)
    m = torch.stack([x, y, z, torch.ones_like(x)], 1)
    for c in range(4):
        for r in range(3):
            T[:, 4 * c + r] = gt[:, r] * m[:, c] + (dW[:, r, c] if c < 3 else 0.0)
    # pixel centre: h = proj (x, y, z, m_w); gscuda (h.x / (h.w + 0.001) * 0.5 + 0.5) W, upstream ((h.x / (h.w + 1e-7) + 1) W - 1) / 2
    mw = torch.ones_like(x) if inria else mw4
    mp = torch.stack([x, y, z, mw], 1)
    eps = float(np.float32(1e-7)) if inria else float(np.float32(0.001))
    hx = pm[0] * x + pm[4] * y + pm[8] * z + pm[12] * mw
    hy = pm[1] * x + pm[5] * y + pm[9] * z + pm[13] * mw
    wp = eps + (pm[3] * x + pm[7] * y + pm[11] * z + pm[15] * mw)
    g2 = _t(dL_dmean2D, dev, F64)[vis]
    ax = 0.5 * width * g2[:, 0] / wp
    ay = 0.5 * height * g2[:, 1] / wp
    aw = -(ax * hx + ay * hy) / wp
    for c in range(4):
        T[:, 16 + 4 * c + 0] = ax * mp[:, c]
        T[:, 16 + 4 * c + 1] = ay * mp[:, c]
        T[:, 16 + 4 * c + 3] = aw * mp[:, c]
    if inria and shs is not None:
        cam = _t(cam_pos, dev, F32).to(F64).reshape(3)
        dv = torch.stack([x, y, z], 1) - cam[None, :]
        ln = torch.sqrt((dv * dv).sum(1))
        d = dv / ln[:, None]
        g = torch.where(_t(clamped, dev, torch.bool)[vis], 0.0, _t(dL_dcolors, dev, F64)[vis])
        sh = _t(shs, dev, F64)[vis].reshape(nv, 16, 3)
        w = (sh * g[:, None, :]).sum(2)                                    # sh[k] . g
        gdir = (_sh_grad_basis(d, min(max(int(sh_degree), 0), 3)) * w[:, :, None]).sum(1)
        T[:, 32:35] = -(gdir - d * (d * gdir).sum(1, keepdim=True)) / ln[:, None]
    return vis, T


def camera_grad(*args, **kw):
    """(g [35], M [35]) as float64 numpy: the camera gradient, and M_k = sum_i |term_ik|, the scale an entry is checked on."""
    _, T = camera_terms(*args, **kw)
    return T.sum(0).cpu().numpy(), T.abs().sum(0).cpu().numpy()


# entries nothing depends on: view row 3, proj row 2
ZERO_ENTRIES = [4 * c + 3 for c in range(4)] + [16 + 4 * c + 2 for c in range(4)]
