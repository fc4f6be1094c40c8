"""What one SplatRasterizer.backward() call computes, where each array's memory comes from and what the caller sees:
the rules alone, as a pure function of the call's choices. No torch and no ctypes: tests/test_backward_plan.py checks every
combination on the CPU. rasterizer.py takes each of these decisions from here and only carries them out."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from types import MappingProxyType

# the per-Gaussian arrays of gsr_backward_args in the order of a full result, with the floats per row
ROW_FLOATS = {"dL_dmean2D": 2, "dL_dconic_opacity": 4, "dL_dcolors": 3, "dL_dcov2D": 4, "dL_dcov3D": 6, "dL_dshs": 48,
              "dL_dmeans3D": 4, "dL_dscales": 4, "dL_drotations": 4}
ARRAYS = tuple(ROW_FLOATS)
SUMS = ARRAYS[:3]                   # what the render backward alone gives: the output set of with_cov3D=False
DEPTHS = "dL_ddepths"               # [N]; beside the nine when a depth gradient is given
CAMERA = ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")
# where an array's memory comes from
INTO, SET, SCRATCH = "into", "set", "scratch"


def output_set(with_cov3D: bool) -> "tuple[str, ...]":
    """The arrays a rasterizer keeps per semantics and hands out: all nine, or the three sums without the chain."""
    return ARRAYS if with_cov3D else SUMS


def depth_mode(depth, last_depth):
    """The depth channel's mode of a backward call: `depth` if given, else that of the last draw(), else True."""
    mode = depth if depth is not None else (last_depth or True)
    assert mode in (True, "inverse"), mode
    return mode


@dataclass(frozen=True)
class BackwardPlan:
    sources: "MappingProxyType[str, str]"   # every array that gets a pointer in gsr_backward_args -> INTO | SET | SCRATCH
    result: "tuple[str, ...]"               # the names of the returned dict, in its order (the camera's three last)
    camera_inputs: "tuple[str, ...]"        # what camera_backward() is handed; () without camera
    camera_into: bool                       # the camera pass writes into["camera"] instead of this object's buffer
    chain_inputs: bool                      # proj_matrix, scales, rotations and scale_modifier are passed
    takes_output_set: bool                  # every call but an into= one holds its semantics' whole set, whatever it points at


@functools.lru_cache(maxsize=None)         # (a caller makes the same few calls every step)
def plan_backward(semantics: str, with_cov3D: bool, wide_sums: bool, outputs: "tuple[str, ...] | None",
                  into: "tuple[str, ...] | None", depth_gradient: bool, camera: bool, colors_precomp: bool) -> BackwardPlan:
    """outputs / into: the names given (into's with "camera" among them or not). Refusals are AssertionErrors.

    - into needs wide_sums and no outputs; its names are among the output set of with_cov3D. outputs needs wide_sums and
      names of that set (dL_ddepths too, beside a depth gradient, where it changes nothing).
    - the result: with into exactly the caller's arrays; with outputs those names; else the whole set. A depth gradient
      adds dL_ddepths to the latter two. dL_ddepths is one buffer per rasterizer kept with the scratch, never the caller's.
    - camera: dL_dmean2D, dL_dcov2D and, for colours from SH (inria, not precomputed), dL_dcolors get pointers whether or not
      the result names them: the result's tensor, else the set's (no into, and the set has it), else scratch. The camera
      pass reads those, and dL_ddepths beside a depth gradient. into["camera"] counts under camera only."""
    assert semantics in ("gscuda", "inria"), semantics
    full = output_set(with_cov3D)
    if into is not None:
        assert wide_sums and outputs is None, "into= needs wide_sums and replaces outputs="
        asked = tuple(k for k in into if k != "camera")
        assert set(asked) <= set(full), sorted(asked)
        sources = dict.fromkeys(asked, INTO)
    elif outputs is not None:
        assert wide_sums and set(outputs) <= set(full + (DEPTHS,) if depth_gradient else full), (outputs, full)
        asked = tuple(dict.fromkeys(outputs))
        sources = dict.fromkeys((k for k in asked if k != DEPTHS), SET)
    else:
        asked = full
        sources = dict.fromkeys(full, SET)
    if depth_gradient:
        sources[DEPTHS] = SCRATCH
        if into is None and DEPTHS not in asked:
            asked += (DEPTHS,)
    camera_inputs = ()
    if camera:
        sh_colour = semantics == "inria" and not colors_precomp      # (colours from SH move with the camera position)
        camera_inputs = ("dL_dmean2D", "dL_dcov2D") + (("dL_dcolors",) if sh_colour else ())
        for k in camera_inputs:
            sources.setdefault(k, SET if into is None and k in full else SCRATCH)
        if depth_gradient:
            camera_inputs += (DEPTHS,)
        asked += CAMERA
    return BackwardPlan(sources=MappingProxyType(sources), result=asked, camera_inputs=camera_inputs,
                        camera_into=camera and into is not None and "camera" in into, chain_inputs=with_cov3D,
                        takes_output_set=into is None)
