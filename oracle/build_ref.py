"""Builds the reference's own CUDA translation units for the host: oracle/_ref/libgscuda_ref.so.

TEST INFRASTRUCTURE (same rules as gsr_oracle.cpp). The recipe
  1. reads apps/gsrast/gscuda/{GSCuda,AuxBuffer,CudaHelpers}.cu of the reference tree (GSR_REFERENCE_DIR, default
     /root/reference),
  2. rewrites every `kernel<<<grid, block>>>(args)` into `::ref_host::launch((grid), (block), kernel, args)` — the only
     change made to the text: the launch configuration is split at its top-level comma and template arguments such as
     `clearColor<3>` stay with the kernel's name — and writes the result into oracle/_ref/,
  3. compiles the three files with the oracle's flags against the stand-in headers of oracle/ref_host/ (CUDA runtime,
     cooperative_groups, cub, glm: the project's own text) and the reference's own .cuh headers, and
  4. links them with oracle/ref_capi.cpp.
Nothing under oracle/_ref/ is committed: the rewritten files are reference text, the library is compiled from it.
Without the reference tree an existing oracle/_ref/ is left as it is (it travels with the working tree to machines that
have no reference tree).
"""
from __future__ import annotations

import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_DIR = os.path.join(HERE, "_ref")
LIB_PATH = os.path.join(OUT_DIR, "libgscuda_ref.so")
UNITS = ("GSCuda", "AuxBuffer", "CudaHelpers")
EXPECTED_LAUNCHES = {"GSCuda": 7, "AuxBuffer": 0, "CudaHelpers": 0}
CXXFLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-pthread"]   # oracle/Makefile's; warnings are the reference's own business


def reference_dir() -> str:
    return os.environ.get("GSR_REFERENCE_DIR", "/root/reference")


def source_dir() -> str:
    return os.path.join(reference_dir(), "apps", "gsrast", "gscuda")


def reference_present() -> bool:
    return all(os.path.isfile(os.path.join(source_dir(), u + ".cu")) for u in UNITS)


def _split_top_level(text: str) -> list[str]:
    parts, depth, start = [], 0, 0
    for i, ch in enumerate(text):
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        elif ch == "," and depth == 0:
            parts.append(text[start:i])
            start = i + 1
    parts.append(text[start:])
    return [p.strip() for p in parts]


_KERNEL_NAME = re.compile(r"([A-Za-z_][A-Za-z_0-9:]*(?:\s*<[^<>;(){}]*>)?)\s*$")


def rewrite_launches(text: str) -> tuple[str, int]:
    """kernel<<<g, b>>>(args) -> ::ref_host::launch((g), (b), kernel, args). Returns the text and the number of launches."""
    out, pos, count = [], 0, 0
    while True:
        lt = text.find("<<<", pos)
        if lt < 0:
            break
        gt = text.find(">>>", lt)
        assert gt > 0, "unterminated launch configuration"
        m = _KERNEL_NAME.search(text, pos, lt)
        assert m, "no kernel name in front of <<<"
        config = _split_top_level(text[lt + 3:gt])
        assert len(config) == 2, f"launch configuration with {len(config)} parts: only <<<grid, block>>> is handled"
        after = gt + 3
        while text[after].isspace():
            after += 1
        assert text[after] == "(", "a launch must be followed by its argument list"
        rest = after + 1
        while text[rest].isspace():
            rest += 1
        assert text[rest] != ")", "a launch without arguments is not handled"
        out.append(text[pos:m.start(1)])
        out.append(f"::ref_host::launch(({config[0]}), ({config[1]}), {m.group(1)}, ")
        pos = after + 1
        count += 1
    out.append(text[pos:])
    return "".join(out), count


def _newer(path: str, than: list[str]) -> bool:
    return os.path.exists(path) and all(os.path.getmtime(path) >= os.path.getmtime(p) for p in than)


def build(force: bool = False, verbose: bool = False) -> str | None:
    """Returns the library's path, or None when there is neither a reference tree nor a library built earlier."""
    if not reference_present():
        return LIB_PATH if os.path.exists(LIB_PATH) else None
    src = source_dir()
    stand_ins = os.path.join(HERE, "ref_host")
    deps = [os.path.join(src, f) for f in os.listdir(src) if f.endswith((".cu", ".cuh"))]
    deps += [os.path.join(d, f) for d, _, fs in os.walk(stand_ins) for f in fs]
    deps += [os.path.join(HERE, "ref_capi.cpp"), os.path.abspath(__file__)]
    if not force and _newer(LIB_PATH, deps):
        return LIB_PATH
    os.makedirs(OUT_DIR, exist_ok=True)
    cxx = os.environ.get("CXX", "g++")
    include = ["-I", stand_ins, "-I", src]
    objects = []
    for unit in UNITS:
        with open(os.path.join(src, unit + ".cu")) as f:
            text, launches = rewrite_launches(f.read())
        assert launches == EXPECTED_LAUNCHES[unit], (unit, launches)
        rewritten = os.path.join(OUT_DIR, unit + ".launches.cpp")
        with open(rewritten, "w") as f:
            f.write(text)
        obj = os.path.join(OUT_DIR, unit + ".o")
        cmd = [cxx, *CXXFLAGS, "-w", *include, "-c", rewritten, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
        objects.append(obj)
    capi = os.path.join(OUT_DIR, "ref_capi.o")
    subprocess.check_call([cxx, *CXXFLAGS, "-Wall", "-Wextra", *include, "-c", os.path.join(HERE, "ref_capi.cpp"), "-o", capi])
    tmp = LIB_PATH + ".tmp"
    subprocess.check_call([cxx, "-shared", "-pthread", "-o", tmp, *objects, capi])
    os.replace(tmp, LIB_PATH)
    if verbose:
        print("built", LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    path = build(force="--force" in sys.argv, verbose=True)
    print(path or "no reference tree and no library built earlier: nothing done")
