"""CPU: the C-ABI library loads, exports every symbol include/gsrast_amd.h declares, and its
host-only entry points (chunk layout, error strings, getHigherMsb) behave like the reference's
(apps/gsrast/gscuda/AuxBuffer.cu:13-21,44-89; GSCuda.cu:481-502). No compute call is made."""
import ctypes as C
import os
import re

import pytest

from helpers import ROOT

from gsrast_amd import _capi
from oracle import cpu_oracle


def _declared_functions():
    text = open(os.path.join(ROOT, "include", "gsrast_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", text)) - {"gsr_alloc_fn"})


def test_library_exports_every_declared_symbol():
    L = _capi.lib()
    names = _declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in gsrast_amd.h but not exported"
    assert set(_capi.SIGNATURES) == set(names), "ctypes table and header disagree"


def test_struct_sizes_match_the_header():
    # gsr_forward refuses a struct whose size differs from the C one; mirror that check host-side
    L = _capi.lib()
    a = _capi.ForwardArgs()
    a.struct_size = C.sizeof(_capi.ForwardArgs) - 4
    assert L.gsr_forward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG
    a.struct_size = C.sizeof(_capi.ForwardArgs)
    assert L.gsr_forward(C.byref(a)) == _capi.GSR_ERR_INVALID_ARG      # null pointers, still no GPU touched
    assert L.gsr_last_error() == _capi.GSR_ERR_INVALID_ARG
    assert b"invalid" in L.gsr_error_string(_capi.GSR_ERR_INVALID_ARG)


def _obtain(off, size, align=128):
    a = align * ((off + align - 1) // align)
    return a, a + size


@pytest.mark.parametrize("n", [1, 1000, 5_834_784])
def test_geometry_chunk_layout_follows_the_reference_carve_order(n):
    """AuxBuffer.cu:44-63: every array 128-byte aligned, in the reference's order and element sizes."""
    L = _capi.lib()
    st = _capi.GeometryState()
    base = 1 << 20
    end = L.gsr_geometry_from_chunk(base, n, C.byref(st))
    off = base
    p, off = _obtain(off, 4 * n); assert st.tiles_touched == p
    p, off = _obtain(off, st.scan_size); assert st.scanning_space == p
    p, off = _obtain(off, 4 * n); assert st.depths == p
    p, off = _obtain(off, 3 * n); assert st.clamped == p
    p, off = _obtain(off, 4 * n); assert st.internal_radii == p
    p, off = _obtain(off, 8 * n); assert st.means2D == p
    p, off = _obtain(off, 24 * n); assert st.cov3D == p
    p, off = _obtain(off, 16 * n); assert st.conic_opacity == p
    p, off = _obtain(off, 12 * n); assert st.rgb == p
    p, off = _obtain(off, 4 * n); assert st.point_offsets == p
    assert end == off
    assert L.gsr_required_geometry(n) == L.gsr_geometry_from_chunk(0, n, C.byref(st))


def test_image_and_binning_chunk_layout():
    L = _capi.lib()
    im = _capi.ImageState()
    P = 1920 * 1080
    end = L.gsr_image_from_chunk(0, P, C.byref(im))
    # uvec2[P], u32[P], f32[P]; 4P is a multiple of 128 here, so no padding (ctypes maps NULL to None)
    assert ((im.ranges or 0), im.n_contrib, im.accum_alpha) == (0, 8 * P, 12 * P)
    assert end == 16 * P == L.gsr_required_image(P)
    b = _capi.BinningState()
    R = 1_000_003
    end = L.gsr_binning_from_chunk(0, R, C.byref(b))
    off = 0
    p, off = _obtain(off, 8 * R); assert (b.keys_unsorted or 0) == p
    p, off = _obtain(off, 8 * R); assert b.keys == p
    p, off = _obtain(off, 4 * R); assert b.values_unsorted == p
    p, off = _obtain(off, 4 * R); assert b.values == p
    p, off = _obtain(off, b.sorting_size); assert b.sorting_space == p
    assert end == off == L.gsr_required_binning(R)


def test_higher_msb_matches_the_reference_values():
    L = _capi.lib()
    for tiles, want in ((64, 7), (3072, 12), (8160, 13), (32400, 15)):
        assert L.gsr_higher_msb(tiles) == want == cpu_oracle.higher_msb(tiles)
    for n in list(range(1, 70000, 37)):
        assert L.gsr_higher_msb(n) == cpu_oracle.higher_msb(n)


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU or PyTorch fallback"):
        _capi.lib()


def _compile_and_run(tmp_path, source: str, flags=(), cxx=False):
    import subprocess
    src = tmp_path / ("probe.cpp" if cxx else "probe.c")
    src.write_text(source)
    exe = tmp_path / "probe"
    cmd = (["g++", "-std=c++17"] if cxx else ["gcc", "-std=c11"]) + ["-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(exe)]
    subprocess.check_call(cmd)
    return subprocess.check_output([str(exe)], text=True)


def test_ctypes_structs_have_the_headers_layout(tmp_path):
    """The header is compiled as C and asked for sizes / offsets; the ctypes mirrors must agree field for field (a
    silent mismatch would shift every pointer behind it)."""
    probes = {"gsr_forward_args": (_capi.ForwardArgs, ["flags", "num_gaussians", "out_color", "stream", "tile_history", "num_rendered",
                                                        "records_staged", "stage_ms", "plan_used", "receipt"]),
              "gsr_backward_args": (_capi.BackwardArgs, ["point_list", "dL_dout_color", "dL_drotations", "stage_ms", "sh_dims",
                                                          "receipt"]),
              "gsr_forward_receipt": (_capi.ForwardReceipt, ["plan_used", "tile_row_end", "num_visible", "serial",
                                                             "geometry_chunk", "binning_chunk", "async_words", "tile_history"])}
    lines = []
    for cname, (_, fields) in probes.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        for f in fields:
            lines.append(f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));')
    out = _compile_and_run(tmp_path, '#include <stdio.h>\n#include <stddef.h>\n#include "gsrast_amd.h"\nint main(void){' + "".join(lines) + "return 0;}")
    got = dict(line.split() for line in out.strip().splitlines())
    for cname, (ctype, fields) in probes.items():
        assert int(got[cname]) == C.sizeof(ctype), cname
        for f in fields:
            assert int(got[f"{cname}.{f}"]) == getattr(ctype, f).offset, f"{cname}.{f}"


def test_python_constants_are_the_headers(tmp_path):
    """Every GSR_FLAG_* / GSR_PLAN_* / GSR_ERR_* the Python mirror names has the header's value (the header compiled as C prints
    them): a flag added on one side only would silently select something else."""
    names = sorted(k for k in vars(_capi) if k.startswith(("GSR_FLAG_", "GSR_PLAN_", "GSR_ERR_")) or k == "GSR_OK")
    assert {"GSR_FLAG_NO_TILE_HISTORY", "GSR_FLAG_SERIAL_EMIT", "GSR_PLAN_EMIT_OVERLAPPED", "GSR_PLAN_COLORS_BESIDE",
            "GSR_PLAN_TILE_ORDER_DROPPED"} <= set(names)
    body = "".join(f'printf("{k} %lld\\n", (long long)({k}));' for k in names)
    out = _compile_and_run(tmp_path, '#include <stdio.h>\n#include "gsrast_amd.h"\nint main(void){' + body + "return 0;}")
    got = dict(line.split() for line in out.strip().splitlines())
    for k in names:
        assert int(got[k]) == int(getattr(_capi, k)), k


def test_poll_async_error_wants_a_receipt():
    L = _capi.lib()
    assert L.gsr_poll_async_error(None) == _capi.GSR_ERR_INVALID_ARG
    assert L.gsr_poll_async_error(C.byref(_capi.ForwardReceipt())) == _capi.GSR_ERR_INVALID_ARG
    # a kernel that gives up writes its call's serial: words {N-sized sort, R-sized sort, owner, 0}
    words = (C.c_uint32 * 4)(7, 0, 7, 0)
    r = _capi.ForwardReceipt()
    r.magic, r.serial, r.async_words = _capi.GSR_RECEIPT_MAGIC, 6, C.addressof(words)
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_ERR_STALE_RECEIPT      # the slot has a new owner: unknown, said so
    r.serial = 7
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_ERR_INTERNAL
    words[0] = 6                                                                  # a late writer of the slot's PREVIOUS owner
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_OK                     # ... does not raise the new owner's flag
    r.serial = 6
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_ERR_INTERNAL           # ... and is still reported to whoever holds its receipt
    words[0], words[1] = 0, 7
    r.serial = 7
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_ERR_INTERNAL
    words[1] = 0
    assert L.gsr_poll_async_error(C.byref(r)) == _capi.GSR_OK


@pytest.mark.parametrize("with_glm", [False, True])
def test_shim_state_pointers_are_glm_typed_when_glm_exists(tmp_path, with_glm):
    """AuxBuffer.cuh:46-49,57 declare glm::vec2* / vec4* / vec3* / uvec2*: with glm on the include path the shim's structs
    carry exactly those types (a caller's `glm::vec2* p = geomState.means2D;` compiles), without it PODs of the same layout.
    This image has no glm; tests/doubles/glm is a stand-in with glm's default layout, for this compile test only."""
    flags = ["-I", os.path.join(ROOT, "tests", "doubles")] if with_glm else []
    body = """
#include <cstdio>
#include <type_traits>
#include "gscuda_shim.hpp"
int main() {
    char* chunk = nullptr;
    gscuda::gs::GeometryState g = gscuda::gs::GeometryState::fromChunk(chunk, 10);
    chunk = nullptr;
    gscuda::gs::ImageState im = gscuda::gs::ImageState::fromChunk(chunk, 64);
#ifdef GSCUDA_SHIM_HAS_GLM
    glm::vec2* m = g.means2D; glm::vec4* c = g.conicOpacity; glm::vec3* rgb = g.rgb; glm::uvec2* r = im.ranges;
    static_assert(std::is_same<gscuda::vec3, glm::vec3>::value, "alias");
    std::printf("glm %d\\n", (int)(m != nullptr && c != nullptr && rgb != nullptr) + (int)(r == nullptr));
#else
    gscuda::vec2* m = g.means2D; (void)m; (void)im;
    std::printf("pod 0\\n");
#endif
    return gscuda::required<gscuda::gs::GeometryState>(10) == gsr_required_geometry(10) ? 0 : 1;
}
"""
    import subprocess
    src = tmp_path / "shim_probe.cpp"
    src.write_text(body)
    exe = tmp_path / "shim_probe"
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), *flags, str(src), "-o", str(exe),
                           _capi.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_capi.LIB_PATH), "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.check_output([str(exe)], text=True)
    assert out.split()[0] == ("glm" if with_glm else "pod")


def test_device_shape_follows_the_compute_unit_count():
    """What the launch heuristics assume about the chip comes from its CU count (hipDeviceAttributeMultiprocessorCount), not
    from constants: a whole MI355X (256 CUs) and one eighth of it (32 CUs, a CPX partition)."""
    L = _capi.lib()
    out = (C.c_uint32 * 4)()
    L.gsr_device_shape(256, out)
    assert list(out) == [256, 5120, 3072, 5120]
    L.gsr_device_shape(32, out)
    assert list(out) == [32, 640, 384, 640]
    L.gsr_device_shape(0, out)                      # (never a division by zero downstream)
    assert out[0] == 1 and out[1] == 20


def test_thread_release_without_any_call_is_a_no_op():
    L = _capi.lib()
    assert L.gsr_thread_release() == _capi.GSR_OK and L.gsr_thread_release() == _capi.GSR_OK


# ---- the error contract of every entry point that returns a GSR_* code (include/gsrast_amd.h, entry_point in csrc/gsr_common.hpp) ----
_NOT_STATUS = {"gsr_last_error", "gsr_exchange_plan"}      # c_int too: the last error itself; a count or a negated code
_AT = 0x10000                                               # an invented, 16-byte aligned address: only in calls of ZERO elements


def _adam_args(rows):
    a = _capi.AdamArgs()
    a.struct_size, a.num_tensors, a.num_rows = C.sizeof(_capi.AdamArgs), 1, rows
    t = a.tensors[0]
    t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.row_floats = _AT, _AT, _AT, _AT, 3
    return C.byref(a)


def _apply_args_of_no_rows():
    a = _capi.DensifyApplyArgs()
    a.struct_size, a.src_of = C.sizeof(_capi.DensifyApplyArgs), _AT                     # (n_src and the four counts: 0)
    for k in ("xyz", "opacity_logit", "log_scale", "rotation", "shs"):
        getattr(a, k).src, getattr(a, k).dst = _AT, _AT
    return C.byref(a)


def _live_receipt():
    """A receipt whose call has nothing to report: words {N-sized sort, R-sized sort, owner, 0} in host memory."""
    words = (C.c_uint32 * 4)(0, 0, 7, 0)
    r = _capi.ForwardReceipt()
    r.magic, r.serial, r.async_words = _capi.GSR_RECEIPT_MAGIC, 7, C.addressof(words)
    r._words = words
    return C.byref(r)


def _ply_header(tmp_path, good):
    p = tmp_path / ("good.ply" if good else "absent.ply")
    if good:
        p.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nend_header\n")
    return (str(p).encode(), C.byref(C.c_int(0)), C.byref(C.c_longlong(0)))


_HOST = (C.c_uint32 * 256)()                                # real, zeroed host memory: refused by its content, never a device address
_HOST_AT = C.addressof(_HOST)
_INVALID = _capi.GSR_ERR_INVALID_ARG
_forward_nulls = lambda _=None: (C.byref(_capi.ForwardArgs(struct_size=C.sizeof(_capi.ForwardArgs))),)
# name -> (arguments that are refused, the code, arguments of a success that makes no HIP call); None: the entry point has no
# such call. A callable is given tmp_path. No row reaches a HIP call: refusals and empty inputs only.
ERROR_CONTRACT = {
    "gsr_forward": (_forward_nulls, _INVALID, None),
    "gsr_backward": ((None,), _INVALID, None),
    "gsr_camera_backward": ((None,), _INVALID, None),
    "gsr_forward_points": ((None,), _INVALID, None),
    "gsr_poll_async_error": ((None,), _INVALID, lambda _: (_live_receipt(),)),
    "gsr_tile_history_create": ((None,), _INVALID, None),
    "gsr_tile_history_destroy": ((_HOST_AT,), _INVALID, (None,)),                      # (zeroed memory is no history: the magic)
    "gsr_tile_history_stats": ((None, None), _INVALID, None),
    "gsr_tile_history_forget_stream": ((None,), _INVALID, None),
    "gsr_tile_history_times": ((None, None, 0, None), _INVALID, None),
    "gsr_thread_release": (None, None, ()),
    "gsr_inclusive_scan_u32": ((None, None, 1, None, None), _INVALID, (None, None, 0, None, None)),
    "gsr_sort_pairs_u64_u32": ((None, None, None, None, 1, 0, 64, None, None), _INVALID, (None, None, None, None, 0, 0, 64, None, None)),
    "gsr_exchange_unique_id": ((None, None), _INVALID, None),
    "gsr_exchange_create": ((None, None, 0, 1, None), _INVALID, None),
    "gsr_exchange_bands": ((None, None, 64, 64, None, -1, None), _INVALID, None),
    "gsr_exchange_loopback": ((None, None, None, 0, 1, None), _INVALID, None),
    "gsr_exchange_destroy": (None, None, (None,)),
    "gsr_ply_parse_header": (lambda tmp: _ply_header(tmp, False), _INVALID, lambda tmp: _ply_header(tmp, True)),
    "gsr_ply_activate": ((None, 1) + (None,) * 6, _INVALID, (_AT, 0) + (_AT,) * 5 + (None,)),
    "gsr_ply_activate_layout": ((None, 1) + (None,) * 5 + (0, None), _INVALID, (_AT, 0) + (_AT,) * 5 + (0, None)),
    "gsr_colors_from_dc": ((1, None, None, None), _INVALID, (0, _AT, _AT, None)),
    "gsr_blend_expf": ((1, None, None, None), _INVALID, (0, _AT, _AT, None)),
    "gsr_footprint_misses_tile": ((1, None, None, None, 16, 16, None, None), _INVALID, (0, _AT, _AT, _AT, 16, 16, _AT, None)),
    "gsr_activate_params": ((1,) + (None,) * 9, _INVALID, (0,) + (_AT,) * 8 + (None,)),
    # (an output asked for — host memory, never reached — without the gradient it is computed from)
    "gsr_activate_params_backward": ((1,) + (None,) * 8 + (_HOST_AT,) + (None,) * 4, _INVALID, (0,) + (_AT,) * 12 + (None,)),
    "gsr_adam_step": (lambda _: (_adam_args(-1),), _INVALID, lambda _: (_adam_args(0),)),
    "gsr_photo_loss_forward": ((None,), _INVALID, None),
    "gsr_photo_loss_backward": ((None,), _INVALID, None),
    "gsr_densify_accumulate": ((1, None, None, 32.0, 32.0, None, None, None, None), _INVALID, (0, _AT, _AT, 32.0, 32.0, _AT, _AT, _AT, None)),
    "gsr_densify_plan": ((1,) + (None,) * 5 + (0.0,) * 5 + (0,) + (None,) * 4, _INVALID, None),   # (n == 0 clears the counts: a HIP call)
    "gsr_densify_apply": ((None,), _INVALID, lambda _: (_apply_args_of_no_rows(),)),
}


def test_the_error_contract_table_names_every_status_returning_entry_point():
    derived = {name for name, (res, _) in _capi.SIGNATURES.items() if res is C.c_int} - _NOT_STATUS
    assert derived == set(ERROR_CONTRACT), sorted(derived ^ set(ERROR_CONTRACT))


@pytest.mark.parametrize("name", sorted(ERROR_CONTRACT))
def test_every_status_returning_entry_point_keeps_the_error_contract(name, tmp_path):
    """A refusal returns its code and leaves it as the last error; a success returns GSR_OK and leaves GSR_OK, directly after
    another entry point was refused; neither leaves a HIP text (none of these calls reaches the HIP runtime)."""
    L = _capi.lib()
    refused, code, fine = ERROR_CONTRACT[name]
    args_of = lambda a: a(tmp_path) if callable(a) else a
    assert refused is not None or fine is not None
    if refused is not None:
        assert L.gsr_tile_history_destroy(None) == _capi.GSR_OK and L.gsr_last_error() == _capi.GSR_OK
        assert getattr(L, name)(*args_of(refused)) == code
        assert L.gsr_last_error() == code and L.gsr_last_hip_error() == b""
    if fine is not None:
        assert L.gsr_forward(*_forward_nulls()) == _INVALID and L.gsr_last_error() == _INVALID
        assert getattr(L, name)(*args_of(fine)) == _capi.GSR_OK
        assert L.gsr_last_error() == _capi.GSR_OK and L.gsr_last_hip_error() == b""
