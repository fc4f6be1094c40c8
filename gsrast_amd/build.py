"""In-tree build of the HIP library: gsrast_amd/csrc/*.hip -> gsrast_amd/lib/libgsrast_amd.so.

gfx950 only, one hipcc invocation per translation unit (cached by mtime), then one link.
The .so stays in the tree (git-ignored) so it travels with the source snapshot to the GPU box.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
OBJ_DIR = os.path.join(LIB_DIR, "obj")
LIB_PATH = os.path.join(LIB_DIR, "libgsrast_amd.so")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"
# -ffp-contract=off: the preprocess / blend arithmetic keeps the reference's float32 operation
# order (no fused multiply-add), which is what makes integer outputs reproducible bit for bit.
COMMON = (["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]
          + os.environ.get("GSR_DEFINES", "").split())      # tuning experiments: GSR_DEFINES="-DX=1 ..."
# Flags of single translation units. antialias.hip: the SLP vectoriser pairs the float32 divisions of the 2D covariance into
# <2 x float> operations, and how it pairs them turns with the shape of the inlined code — one division formed twice, packed moves
# around every pair. Its kernels are bound by their double arithmetic and their memory; without the pass they are shorter and keep
# half the registers in the forward (no result changes: nothing is reassociated). profiles/chain_passes_cost.txt has the times.
PER_FILE = {"antialias.hip": ["-fno-slp-vectorize"]}


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))


def _headers_mtime() -> float:
    paths = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".h"))]
    paths += [os.path.join(HERE, "..", "include", h) for h in ("gsrast_amd.h", "gsrast_amd_init.h", "gsrast_amd_opacity.h", "gsrast_amd_mcmc.h",
                                                                      "gsrast_amd_contrib.h", "gsrast_amd_antialias.h", "gsrast_amd_filter3d.h", "gsrast_amd_absgrad.h",
                                                                      "gsrast_amd_features.h", "gsrast_amd_distortion.h", "gsrast_amd_normals.h", "gsrast_amd_median.h")]
    return max(os.path.getmtime(p) for p in paths)


def _compile(src: str, force: bool, obj_dir: str = OBJ_DIR) -> str:
    obj = os.path.join(obj_dir, src[:-4] + ".o")
    spath = os.path.join(CSRC, src)
    stale = (force or not os.path.exists(obj) or os.path.getmtime(obj) < os.path.getmtime(spath)
             or os.path.getmtime(obj) < _headers_mtime())
    if stale:
        cmd = [HIPCC] + COMMON + PER_FILE.get(src, []) + ["-c", spath, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip():
            sys.stderr.write(r.stderr)
    return obj


def build(force: bool = False, verbose: bool = False, tag: str = "") -> str:
    """tag: experiments only — builds lib/libgsrast_amd_<tag>.so from its own object directory
    (always from scratch, with whatever GSR_DEFINES is set), selected at run time by GSR_LIB_TAG."""
    obj_dir = OBJ_DIR + ("_" + tag if tag else "")
    lib_path = LIB_PATH if not tag else os.path.join(LIB_DIR, f"libgsrast_amd_{tag}.so")
    force = force or bool(tag)
    os.makedirs(obj_dir, exist_ok=True)
    srcs = _sources()
    with ThreadPoolExecutor(max_workers=min(4, len(srcs))) as ex:
        objs = list(ex.map(lambda s: _compile(s, force, obj_dir), srcs))
    newest = max(os.path.getmtime(o) for o in objs)
    if force or not os.path.exists(lib_path) or os.path.getmtime(lib_path) < newest:
        cmd = [HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib_path] + objs + ["-ldl"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    if verbose:
        print("built", lib_path)
    return lib_path


if __name__ == "__main__":
    _tag = sys.argv[sys.argv.index("--tag") + 1] if "--tag" in sys.argv else ""
    build(force="--force" in sys.argv, verbose=True, tag=_tag)
