"""The reference of gsr_knn_mean_dist2 (include/gsrast_amd_init.h): the definition itself as a brute force over all pairs, in
numpy, chunked over the query rows. In float32 it states what the kernels must give bit for bit; in float64 it bounds the
float32 one (tests/test_knn_cpu.py). Nothing here orders or prunes anything: no grid, no tree, no code.

morton_order is a 30-bit Morton order (10 bits an axis, upstream's) that serves one purpose: the guards of the test scenes,
which show on an order that is NOT the library's that a search along a sorted order alone would miss true neighbours.
"""
import numpy as np

CHUNK = 512


def nearest(xyz, dtype=np.float32):
    """(d2 [n,k] ascending, idx [n,k]) with k = min(3, n - 1): the k smallest d2(i, j), j != i (INDICES are compared: a
    duplicate of row i is a neighbour at distance 0), and rows that attain them. d2 = (dx*dx + dy*dy) + dz*dz in `dtype`."""
    p = np.ascontiguousarray(xyz, dtype)
    n = p.shape[0]
    k = min(3, n - 1)
    d2_out, idx_out = np.empty((n, k), dtype), np.empty((n, k), np.int64)
    if k == 0:
        return d2_out, idx_out
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    for at in range(0, n, CHUNK):
        rows = slice(at, min(at + CHUNK, n))
        dx, dy, dz = x[rows, None] - x[None, :], y[rows, None] - y[None, :], z[rows, None] - z[None, :]
        d2 = (dx * dx + dy * dy) + dz * dz
        assert d2.dtype == dtype
        d2[np.arange(rows.stop - rows.start), np.arange(rows.start, rows.stop)] = np.inf
        if n - 1 > k:
            part = np.argpartition(d2, k - 1, axis=1)[:, :k]
        else:
            part = np.argsort(d2, axis=1)[:, :k]
        vals = np.take_along_axis(d2, part, axis=1)
        order = np.argsort(vals, axis=1, kind="stable")
        d2_out[rows] = np.take_along_axis(vals, order, axis=1)
        idx_out[rows] = np.take_along_axis(part, order, axis=1)
    return d2_out, idx_out


def mean_of(d2, n):
    """mean_dist2 from the ascending k smallest distances, in their dtype: ((b0 + b1) + b2) / 3, (b0 + b1) / 2, b0, +0."""
    t = d2.dtype.type
    if n >= 4:
        return ((d2[:, 0] + d2[:, 1]) + d2[:, 2]) / t(3)
    if n == 3:
        return (d2[:, 0] + d2[:, 1]) / t(2)
    if n == 2:
        return d2[:, 0].copy()
    return np.zeros(n, d2.dtype)


def mean_dist2(xyz, dtype=np.float32):
    xyz = np.asarray(xyz)
    return mean_of(nearest(xyz, dtype)[0], xyz.shape[0])


def _spread10(v):
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def morton_order(xyz):
    """The rows of xyz in the order of a 30-bit Morton code over their bounding box (stable); a zero-extent axis is cell 0."""
    p = np.asarray(xyz, np.float64)
    lo, extent = p.min(0), p.max(0) - p.min(0)
    cells = np.where(extent > 0, (p - lo) / np.where(extent > 0, extent, 1.0) * 1023.0, 0.0).astype(np.uint32)
    code = _spread10(cells[:, 0]) | (_spread10(cells[:, 1]) << np.uint32(1)) | (_spread10(cells[:, 2]) << np.uint32(2))
    return np.argsort(code, kind="stable")


def farthest_neighbour_places(xyz, idx):
    """Per row: how many places its farthest true neighbour (idx of nearest()) lies away in morton_order."""
    order = morton_order(xyz)
    place = np.empty(order.shape[0], np.int64)
    place[order] = np.arange(order.shape[0])
    return np.abs(place[idx] - place[:, None]).max(axis=1)
