"""CPU: gsrast_amd/backward_plan.py, the rules of SplatRasterizer.backward() — which arrays get a pointer, whose memory each
is, what the caller sees, what the camera pass is handed — over the full product of the call's choices. The rules are
written out here on their own; nothing is derived from a second call of the planner."""
import itertools
import os
import subprocess
import sys

import pytest

from gsrast_amd import backward_plan as P

NINE = ("dL_dmean2D", "dL_dconic_opacity", "dL_dcolors", "dL_dcov2D", "dL_dcov3D", "dL_dshs", "dL_dmeans3D", "dL_dscales",
        "dL_drotations")
THREE = ("dL_dmean2D", "dL_dconic_opacity", "dL_dcolors")
CAM_KEYS = ("dL_dview_matrix", "dL_dproj_matrix", "dL_dcam_pos")
CONFIG5 = ("dL_dmean2D", "dL_dcov3D", "dL_dshs")                      # BASELINE config 5
INPUTS = ("dL_dmean2D", "dL_dconic_opacity", "dL_dshs", "dL_dmeans3D", "dL_dscales", "dL_drotations")
LISTS = (CONFIG5, INPUTS) + tuple((k,) for k in NINE)
# (kind, names, "camera" among into's names)
SELECTIONS = ([("all", None, False)] + [("outputs", names, False) for names in LISTS]
              + [("into", names, cam_key) for names in LISTS for cam_key in (False, True)])


def _plan(semantics, cov, wide, kind, names, cam_key, depth, camera, precomp):
    outputs = names if kind == "outputs" else None
    into = (names + (("camera",) if cam_key else ())) if kind == "into" else None
    return P.plan_backward(semantics, cov, wide, outputs, into, depth, camera, precomp)


def test_the_module_needs_neither_torch_nor_ctypes():
    code = ("import sys; from gsrast_amd import backward_plan as P; "
            "P.plan_backward('gscuda', True, True, None, None, True, True, False); "
            "assert 'torch' not in sys.modules and 'ctypes' not in sys.modules and 'numpy' not in sys.modules")
    subprocess.check_call([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_the_names_are_those_of_the_abi():
    assert P.ARRAYS == NINE and P.SUMS == THREE and P.CAMERA == CAM_KEYS and P.DEPTHS == "dL_ddepths"
    assert P.ROW_FLOATS == {"dL_dmean2D": 2, "dL_dconic_opacity": 4, "dL_dcolors": 3, "dL_dcov2D": 4, "dL_dcov3D": 6,
                            "dL_dshs": 48, "dL_dmeans3D": 4, "dL_dscales": 4, "dL_drotations": 4}
    assert P.output_set(True) == NINE and P.output_set(False) == THREE


@pytest.mark.parametrize("semantics,cov,wide,depth,camera,precomp",
                         list(itertools.product(("gscuda", "inria"), (True, False), (True, False), (True, False),
                                                (True, False), (True, False))))
def test_every_combination_follows_the_rules(semantics, cov, wide, depth, camera, precomp):
    own_set = NINE if cov else THREE
    for kind, names, cam_key in SELECTIONS:
        args = (semantics, cov, wide, kind, names, cam_key, depth, camera, precomp)
        # refusals: outputs / into need the double sums, and names of the set the call's with_cov3D gives
        if kind != "all" and (not wide or not set(names) <= set(own_set)):
            with pytest.raises(AssertionError):
                _plan(*args)
            continue
        p = _plan(*args)
        # the result: names and order
        per_gaussian = own_set if kind == "all" else names
        if depth and kind != "into":
            per_gaussian += ("dL_ddepths",)
        assert p.result == per_gaussian + (CAM_KEYS if camera else ()), args
        # what the camera pass reads, and with it what gets a pointer
        cam_in = ()
        if camera:
            cam_in = ("dL_dmean2D", "dL_dcov2D")
            if semantics == "inria" and not precomp:
                cam_in += ("dL_dcolors",)
            if depth:
                cam_in += ("dL_ddepths",)
        assert p.camera_inputs == cam_in, args
        pointers = set(p.sources)
        assert pointers >= set(per_gaussian) and pointers >= set(cam_in), args
        assert pointers == set(per_gaussian) | set(cam_in) | ({"dL_ddepths"} if depth else set()), args
        if not cov:
            assert not pointers & {"dL_dcov3D", "dL_dshs", "dL_dmeans3D", "dL_dscales", "dL_drotations"}, args
        # whose memory
        for k, source in p.sources.items():
            if kind == "into":
                assert source == ("into" if k in names else "scratch"), (args, k)
            else:
                assert source == ("set" if k in own_set else "scratch"), (args, k)     # (dL_ddepths; dL_dcov2D without the chain)
        assert p.takes_output_set == (kind != "into"), args
        assert p.camera_into == (camera and kind == "into" and cam_key), args
        assert p.chain_inputs == cov, args


def test_refusals():
    plan = P.plan_backward
    for bad in (dict(outputs=CONFIG5, into=CONFIG5),                      # into replaces outputs
                dict(into=("dL_dmean2D", "dL_dnothing")), dict(outputs=("dL_dnothing",)),
                dict(into=("dL_ddepths",), depth_gradient=True),          # scratch of this object, never the caller's
                dict(outputs=("dL_ddepths",)),                            # there is none without a depth gradient
                dict(into=("dL_dcov2D",), with_cov3D=False), dict(outputs=("dL_dcov3D",), with_cov3D=False),
                dict(outputs=("dL_dcov3D",), wide_sums=False), dict(into=("dL_dmean2D",), wide_sums=False),
                dict(semantics="other")):
        kw = dict(semantics="gscuda", with_cov3D=True, wide_sums=True, outputs=None, into=None, depth_gradient=False,
                  camera=False, colors_precomp=False)
        kw.update(bad)
        with pytest.raises(AssertionError):
            plan(**kw)


def test_the_cases_of_the_camera_plumbing_test():
    """tests/test_gpu_camera_grad.py::test_camera_grad_plumbing_of_outputs_and_with_cov3D, with a depth gradient throughout."""
    few = P.plan_backward("gscuda", True, True, ("dL_dcov3D",), None, True, True, False)
    assert few.result == ("dL_dcov3D", "dL_ddepths") + CAM_KEYS
    assert dict(few.sources) == {"dL_dcov3D": "set", "dL_ddepths": "scratch", "dL_dmean2D": "set", "dL_dcov2D": "set"}
    assert few.camera_inputs == ("dL_dmean2D", "dL_dcov2D", "dL_ddepths")
    bare = P.plan_backward("gscuda", False, True, None, None, True, True, False)
    assert bare.result == THREE + ("dL_ddepths",) + CAM_KEYS and not bare.chain_inputs
    assert bare.sources["dL_dcov2D"] == "scratch" and bare.camera_inputs == ("dL_dmean2D", "dL_dcov2D", "dL_ddepths")
    plain = P.plan_backward("gscuda", True, True, None, None, True, False, False)
    assert plain.result == NINE + ("dL_ddepths",) and plain.camera_inputs == ()


@pytest.mark.parametrize("subset", [("dL_dmean2D", "dL_dcov3D", "dL_dshs"),
                                    ("dL_dmean2D", "dL_dconic_opacity", "dL_dshs", "dL_dmeans3D", "dL_dscales", "dL_drotations"),
                                    ("dL_dmeans3D",), ("dL_dcolors",), ("dL_dshs",)])
def test_the_subsets_of_the_optional_outputs_test(subset):
    """tests/test_gpu_backward.py::test_optional_outputs_give_the_same_numbers_and_leave_the_others_alone: exactly the
    subset is returned and exactly the subset is written."""
    p = P.plan_backward("gscuda", True, True, subset, None, False, False, False)
    assert p.result == subset and dict(p.sources) == dict.fromkeys(subset, "set")
    assert p.chain_inputs and p.takes_output_set and p.camera_inputs == ()


def test_the_trainers_into_call():
    """What gsrast_amd.autograd asks for with camera tensors and a depth loss: the caller's five and nothing of the sets."""
    five = ("dL_dmeans3D", "dL_dscales", "dL_drotations", "dL_dconic_opacity", "dL_dshs")
    p = P.plan_backward("inria", True, True, None, five + ("camera",), True, True, False)
    assert p.result == five + CAM_KEYS and p.camera_into and not p.takes_output_set
    assert {k for k, s in p.sources.items() if s == "scratch"} == {"dL_ddepths", "dL_dmean2D", "dL_dcov2D", "dL_dcolors"}
    assert "set" not in p.sources.values()
    # into["camera"] without camera=True is ignored
    q = P.plan_backward("inria", True, True, None, five + ("camera",), False, False, False)
    assert q.result == five and not q.camera_into and dict(q.sources) == dict.fromkeys(five, "into")


def test_duplicate_names_and_dL_ddepths_among_outputs():
    p = P.plan_backward("gscuda", True, True, ("dL_dshs", "dL_ddepths", "dL_dshs"), None, True, False, False)
    assert p.result == ("dL_dshs", "dL_ddepths") and dict(p.sources) == {"dL_dshs": "set", "dL_ddepths": "scratch"}


def test_depth_mode():
    assert P.depth_mode(None, False) is True and P.depth_mode(None, True) is True
    assert P.depth_mode(None, "inverse") == "inverse" and P.depth_mode(True, "inverse") is True
    assert P.depth_mode("inverse", False) == "inverse"
    for bad in (False, "linear", 1.5):
        with pytest.raises(AssertionError):
            P.depth_mode(bad, True)


def test_a_plan_cannot_be_changed():
    p = P.plan_backward("gscuda", True, True, None, None, False, False, False)
    with pytest.raises(Exception):
        p.result = ()
    with pytest.raises(TypeError):
        p.sources["dL_dshs"] = "into"
