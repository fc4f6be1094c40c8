"""Mints tests/golden/reference_frames.npz: the inputs of a handful of tiny frames and every output the reference binary
wrote for them — oracle/_ref/libgscuda_ref.so, the reference's own GSCuda.cu / AuxBuffer.cu / CudaHelpers.cu compiled for the
host (oracle/build_ref.py; needs the reference tree). The file holds data only: what the binary read and what it wrote.

tests/test_reference_pin.py checks both oracles against the record (anywhere) and the record against a fresh run of the
binary (where it can be built). Run from the repo root:  python tests/golden/make_reference_frames.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import reference_frames as F                   # noqa: E402
from oracle import ref_cpu                     # noqa: E402


def frames():
    yield "anisotropic_48x32", F.anisotropic(48, 32, 160, 3)
    scene, cam, bg, kw = F.anisotropic(48, 32, 160, 3)
    yield "radius_path_scale_0.6", (scene, cam, bg, dict(kw, use_rects=False, scale_modifier=0.6))
    yield "single_tile_column_14x263", F.random_small_frame(1)
    yield "single_instance", F.single_instance()
    yield "nothing_visible", F.nothing_visible()
    yield "precomputed_colours_and_covariances", F.precomputed_inputs(True, True, 48, 32, 160)


def main():
    out = {}
    names = []
    for name, (scene, cam, bg, kw) in frames():
        ref = ref_cpu.forward(scene, cam, bg, **kw)
        assert F.conversions_in_range(ref, cam).all(), name
        assert not scene["shs"][:, 3:].any(), name           # (only the DC triple is stored)
        p = name + "/"
        for k in ("means3D", "scales", "rotations", "opacities"):
            out[p + "in_" + k] = np.asarray(scene[k], np.float32)
        out[p + "in_shs_dc"] = np.asarray(scene["shs"][:, :3], np.float32).copy()
        for k in ("colors_precomp", "cov3d_precomp", "out_init"):
            if k in kw:
                out[p + "in_" + k] = np.asarray(kw[k], np.float32)
        out[p + "use_rects"] = np.array(kw.get("use_rects", True))
        out[p + "scale_modifier"] = np.array(kw.get("scale_modifier", 1.0), np.float32)
        out.update({p + "cam_view": cam.view, p + "cam_proj": cam.proj, p + "cam_pos": cam.cam_pos,
                    p + "cam_tan": np.array([cam.tan_fovx, cam.tan_fovy], np.float32),
                    p + "size": np.array([cam.width, cam.height], np.int32), p + "background": np.array(bg, np.float32),
                    p + "num_rendered": np.array(ref["num_rendered"], np.int64)})
        for k in F.REF_KEYS:
            if ref[k] is not None:
                out[p + "exp_" + k] = ref[k]
        names.append(name)
        print(f"{name}: {cam.width}x{cam.height} N={scene['means3D'].shape[0]} R={ref['num_rendered']}")
    out["frames"] = np.array(names)
    path = os.path.join(ROOT, "tests", "golden", "reference_frames.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size <= 297 * 1024, "larger than tests/golden/config1.npz: drop a frame"


if __name__ == "__main__":
    main()
