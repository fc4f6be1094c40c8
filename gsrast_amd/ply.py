"""3DGS .ply scene loading: the role of `SplatData` in the reference
(apps/gsrast/SplatData.{hpp,cpp}). Header parsing and file I/O happen on the host exactly as
the reference does them; the per-splat activations run on the GPU (`gsr_ply_activate`).

File format (SplatData.hpp:17-25, SplatData.cpp:114-156): after the header, N records of 62
little-endian float32 — position 3, normal 3, f_dc/f_rest 48, opacity 1, scale 3, rotation 4 —
in that fixed order; property names in the header are not interpreted.

`read_points_ply` reads the other .ply of a 3DGS data set, the SfM point cloud a training run starts from (upstream's
points3D.ply): there the properties ARE found by name.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi

RECORD_FLOATS = 62


def parse_header(path: str) -> tuple[int, int]:
    """(vertex count, byte offset of the first record). Raises on an unreadable header."""
    n, off = C.c_int(0), C.c_longlong(0)
    rc = _capi.lib().gsr_ply_parse_header(path.encode(), C.byref(n), C.byref(off))
    if rc != _capi.GSR_OK or off.value < 0:
        raise ValueError(f"{path}: not a readable .ply header (no end_header line)")
    return int(n.value), int(off.value)


def load_ply(path: str, device="cuda:0", sh_layout: str = "file") -> dict:
    """Loads a scene to the device in the layout `SplatRasterizer.configure_from_scene` takes.
    Also returns the bounding box and centre the reference computes (SplatData.cpp:55-62).

    sh_layout: "file" keeps the 48 SH floats as they lie in the file (f_dc, then f_rest channel-major) — what the
    reference does, and all its DC-only colour needs; "coefficient_major" transposes f_rest to [16][3], the layout
    `draw(semantics="inria", sh_degree >= 1)` reads (GSR_SH_LAYOUT_*, include/gsrast_amd.h)."""
    layout = {"file": _capi.GSR_SH_LAYOUT_FILE, "coefficient_major": _capi.GSR_SH_LAYOUT_COEFFICIENT_MAJOR}[sh_layout]
    n, off = parse_header(path)
    raw = np.fromfile(path, dtype="<f4", offset=off, count=n * RECORD_FLOATS)
    if raw.size < n * RECORD_FLOATS:                  # the reference rejects a short file (:147-152)
        raise ValueError(f"{path}: file ends before {n} records")
    dev = torch.device(device)
    raw_dev = torch.from_numpy(raw).to(dev)
    out = {
        "means3D": torch.empty((n, 4), dtype=torch.float32, device=dev),
        "scales": torch.empty((n, 4), dtype=torch.float32, device=dev),
        "rotations": torch.empty((n, 4), dtype=torch.float32, device=dev),
        "opacities": torch.empty((n,), dtype=torch.float32, device=dev),
        "shs": torch.empty((n, 48), dtype=torch.float32, device=dev),
    }
    _capi.call("gsr_ply_activate_layout", raw_dev.data_ptr(), n, out["means3D"].data_ptr(), out["scales"].data_ptr(),
               out["rotations"].data_ptr(), out["opacities"].data_ptr(), out["shs"].data_ptr(), layout, _capi.stream(dev), device=dev)
    out["sh_layout"] = sh_layout
    torch.cuda.current_stream(dev).synchronize()
    pos = out["means3D"][:, :3]
    out["bbox_min"], out["bbox_max"] = pos.min(0).values, pos.max(0).values
    out["center"] = pos.mean(0)
    return out


_POINT_TYPES = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "char": "i1",
                "int8": "i1", "short": "<i2", "int16": "<i2", "ushort": "<u2", "uint16": "<u2", "int": "<i4", "int32": "<i4",
                "uint": "<u4", "uint32": "<u4"}


def read_points_ply(path: str):
    """(xyz float32 [N,3], rgb uint8 [N,3]) of a point cloud in the layout of upstream's points3D.ply: binary little
    endian, one `vertex` element with float x y z, optionally float nx ny nz, and uchar red green blue. Properties are
    found by NAME in the header, so their order and further scalar properties do not matter. ValueError, naming what is
    missing: no header, another format (ascii), no vertex element, a list property, x/y/z not float or red/green/blue not
    uchar or not there, a file that ends before the last vertex."""
    with open(path, "rb") as f:
        head = f.read(1 << 16)
    end = head.find(b"end_header\n")
    if not head.startswith(b"ply") or end < 0:
        raise ValueError(f"{path}: not a .ply file (no 'ply' ... 'end_header' header)")
    offset = end + len(b"end_header\n")
    lines = [l.split() for l in head[:end].decode("ascii", "replace").splitlines()]
    fmt = [l for l in lines if l and l[0] == "format"]
    if not fmt or fmt[0][1:2] != ["binary_little_endian"]:
        raise ValueError(f"{path}: format {' '.join(fmt[0][1:]) if fmt else '(none)'}, not binary_little_endian")
    n, fields, element = None, [], None
    for l in lines:
        if l and l[0] == "element":
            element = l[1] if len(l) > 1 else None
            if element == "vertex":
                n = int(l[2])
            elif n is None:
                raise ValueError(f"{path}: element {element} stands before the vertex element")
        elif l and l[0] == "property" and element == "vertex":
            if len(l) != 3 or l[1] not in _POINT_TYPES:
                raise ValueError(f"{path}: vertex property '{' '.join(l[1:])}' is not a scalar of a known type")
            fields.append((l[2], _POINT_TYPES[l[1]]))
    if n is None:
        raise ValueError(f"{path}: no vertex element")
    types = dict(fields)
    for names, want, said in ((("x", "y", "z"), "<f4", "float"), (("red", "green", "blue"), "u1", "uchar")):
        missing = [k for k in names if k not in types]
        if missing:
            raise ValueError(f"{path}: no vertex property {', '.join(missing)}")
        wrong = [k for k in names if types[k] != want]
        if wrong:
            raise ValueError(f"{path}: vertex property {', '.join(wrong)} is not {said}")
    if len(types) != len(fields):
        raise ValueError(f"{path}: a vertex property is declared twice")
    rec = np.fromfile(path, dtype=np.dtype(fields), offset=offset, count=n)
    if rec.shape[0] < n:
        raise ValueError(f"{path}: file ends before {n} vertices")
    xyz = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    rgb = np.stack([rec["red"], rec["green"], rec["blue"]], axis=1).astype(np.uint8)
    return xyz, rgb


def write_ply(path: str, position, sh, opacity_logit, log_scale, rotation, normal=None) -> None:
    """Writes a scene in the standard 3DGS property order (used by tests and tools)."""
    position = np.asarray(position, np.float32)
    n = position.shape[0]
    rec = np.zeros((n, RECORD_FLOATS), np.float32)
    rec[:, 0:3] = position
    if normal is not None:
        rec[:, 3:6] = normal
    rec[:, 6:54] = np.asarray(sh, np.float32).reshape(n, 48)
    rec[:, 54] = opacity_logit
    rec[:, 55:58] = log_scale
    rec[:, 58:62] = rotation
    props = (["x", "y", "z", "nx", "ny", "nz"] + [f"f_dc_{i}" for i in range(3)] + [f"f_rest_{i}" for i in range(45)]
             + ["opacity"] + [f"scale_{i}" for i in range(3)] + [f"rot_{i}" for i in range(4)])
    header = "ply\nformat binary_little_endian 1.0\nelement vertex %d\n" % n
    header += "".join(f"property float {p}\n" for p in props) + "end_header\n"
    with open(path, "wb") as f:
        f.write(header.encode())
        f.write(rec.astype("<f4").tobytes())
