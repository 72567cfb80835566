"""The lightmap finish's pass plan, host side (CPU only): cs397raytracingsp22_amd/csrc/render_plan.cpp finish_plan — which buffer the
initial step and every pass of mi_lightmap_finish, mi_lightmap_finish_sh and mi_lightmap_finish_var reads and writes — asked through
tests/cpp/render_plan_shim.cpp, no GPU and no libmi_rt.so.  The written-out plans spell every slot from the rules in render_plan.hpp;
the invariants run over every (levels, dilate, flags) the entry points accept at their edges."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs397raytracingsp22_amd", "csrc")
IN, OUT, P0, P1 = 0, 1, 2, 3               # image slots: the caller's input and output, the two ping images
M0, M1, MC = 0, 1, 2                       # mask slots: the two ping masks, the caller's
V0, V1, VC = 0, 1, 2                       # variance slots: the two ping planes, the caller's
NONE = 3                                   # a mask / variance slot the step does not touch
MAX_PASSES = 8 + 256


class FinishPlanQuery(C.Structure):        # tests/cpp/render_plan_shim.cpp
    _fields_ = [("levels", C.c_uint32), ("dilate", C.c_uint32), ("want_valid", C.c_int32), ("with_var", C.c_int32), ("want_var", C.c_int32),
                ("copy", C.c_uint32), ("mask_init", C.c_uint32), ("var_init", C.c_uint32),
                ("passes", C.POINTER(C.c_uint32)), ("passes_cap", C.c_uint32)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("fp") / "render_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-shared",
                    os.path.join(CSRC, "render_plan.cpp"), os.path.join(CSRC, "scene_compile.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "render_plan_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.finish_plan_query.argtypes = [C.POINTER(FinishPlanQuery)]
    lib.finish_plan_query.restype = C.c_int
    words = (C.c_uint32 * (8 * MAX_PASSES))()

    def plan(levels, dilate, want_valid=False, with_var=False, want_var=False):
        """(copy, mask_init, var_init), [(level, step, image in, image out, mask in, mask out, variance in, variance out), ...]"""
        q = FinishPlanQuery(levels=levels, dilate=dilate, want_valid=want_valid, with_var=with_var, want_var=want_var,
                            passes=words, passes_cap=MAX_PASSES)
        n = lib.finish_plan_query(C.byref(q))
        assert n >= 0
        return (q.copy, q.mask_init, q.var_init), [tuple(words[8 * p:8 * p + 8]) for p in range(n)]
    return plan


def level(step, src, dst, var_in=NONE, var_out=NONE):
    return (1, step, src, dst, NONE, NONE, var_in, var_out)


def dilation(src, dst, mask_in, mask_out):
    return (0, 0, src, dst, mask_in, mask_out, NONE, NONE)


# ---------------------------------------------------------------------------------------------- written-out plans
def test_no_pass_at_all_copies_into_the_output(plan):
    assert plan(0, 0) == ((1, M0, NONE), [])
    assert plan(0, 0, want_valid=True) == ((1, MC, NONE), [])
    assert plan(0, 0, with_var=True) == ((1, M0, V0), [])
    assert plan(0, 0, with_var=True, want_var=True) == ((1, M0, VC), [])
    assert plan(0, 0, want_valid=True, with_var=True, want_var=True) == ((1, MC, VC), [])
    assert plan(0, 0, want_valid=True, with_var=True) == ((1, MC, V0), [])


def test_one_level(plan):
    assert plan(1, 0) == ((0, M0, NONE), [level(1, IN, OUT)])
    assert plan(1, 0, want_valid=True) == ((0, MC, NONE), [level(1, IN, OUT)])
    assert plan(1, 0, with_var=True) == ((0, M0, V0), [level(1, IN, OUT, V0, V1)])
    assert plan(1, 0, want_valid=True, with_var=True, want_var=True) == ((0, MC, V0), [level(1, IN, OUT, V0, VC)])


def test_one_dilation(plan):
    assert plan(0, 1) == ((0, M0, NONE), [dilation(IN, OUT, M0, M1)])
    assert plan(0, 1, want_valid=True) == ((0, M0, NONE), [dilation(IN, OUT, M0, MC)])
    assert plan(0, 1, with_var=True) == ((0, M0, V0), [dilation(IN, OUT, M0, M1)])
    assert plan(0, 1, want_valid=True, with_var=True, want_var=True) == ((0, M0, VC), [dilation(IN, OUT, M0, MC)])


def test_two_levels_and_a_dilation(plan):
    assert plan(2, 1) == ((0, M0, NONE), [level(1, IN, P0), level(2, P0, P1), dilation(P1, OUT, M0, M1)])
    assert plan(2, 1, want_valid=True, with_var=True, want_var=True) == (
        (0, M0, V0), [level(1, IN, P0, V0, V1), level(2, P0, P1, V1, VC), dilation(P1, OUT, M0, MC)])
    assert plan(2, 1, with_var=True) == (
        (0, M0, V0), [level(1, IN, P0, V0, V1), level(2, P0, P1, V1, V0), dilation(P1, OUT, M0, M1)])


def test_three_levels_and_two_dilations(plan):
    assert plan(3, 2) == ((0, M0, NONE), [level(1, IN, P0), level(2, P0, P1), level(4, P1, P0),
                                          dilation(P0, P1, M0, M1), dilation(P1, OUT, M1, M0)])
    assert plan(3, 2, want_valid=True, with_var=True, want_var=True) == (
        (0, M0, V0), [level(1, IN, P0, V0, V1), level(2, P0, P1, V1, V0), level(4, P1, P0, V0, VC),
                      dilation(P0, P1, M0, M1), dilation(P1, OUT, M1, MC)])


def test_one_level_and_three_dilations(plan):
    assert plan(1, 3) == ((0, M0, NONE), [level(1, IN, P0), dilation(P0, P1, M0, M1), dilation(P1, P0, M1, M0),
                                          dilation(P0, OUT, M0, M1)])
    assert plan(1, 3, want_valid=True, with_var=True, want_var=True) == (
        (0, M0, V0), [level(1, IN, P0, V0, VC), dilation(P0, P1, M0, M1), dilation(P1, P0, M1, M0), dilation(P0, OUT, M0, MC)])


# ---------------------------------------------------------------------------------------------- invariants
GRID = [(levels, dilate, want_valid, with_var, want_var)
        for levels in range(9) for dilate in (0, 1, 2, 3, 255, 256)
        for want_valid, with_var, want_var in itertools.product((False, True), repeat=3)]


def test_invariants_over_the_accepted_range(plan):
    for levels, dilate, want_valid, with_var, want_var in GRID:
        (copy, mask_init, var_init), passes = plan(levels, dilate, want_valid, with_var, want_var)
        case = (levels, dilate, want_valid, with_var, want_var)
        # levels + dilate passes, the levels first, at steps 1, 2, 4, ...
        assert len(passes) == levels + dilate, case
        assert [(p[0], p[1]) for p in passes] == [(1, 1 << p) for p in range(levels)] + [(0, 0)] * dilate, case
        assert copy == (0 if passes else 1), case
        # every pass reads what the previous one wrote, in all three kinds; none reads and writes the same slot
        image, mask, var = IN, mask_init, var_init
        image_writes, mask_writes, var_writes = ([OUT] if copy else []), [mask_init], [var_init]
        assert mask_init != NONE and (var_init != NONE) == with_var, case
        for is_level, _, src, dst, mask_in, mask_out, var_in, var_out in passes:
            assert src == image and src != dst, case
            image = dst
            image_writes.append(dst)
            if is_level:
                assert (mask_in, mask_out) == (NONE, NONE), case
                if with_var:
                    assert var_in == var and var_out not in (var_in, NONE), case
                    var = var_out
                    var_writes.append(var_out)
                else:
                    assert (var_in, var_out) == (NONE, NONE), case
            else:
                assert (var_in, var_out) == (NONE, NONE), case         # the dilations leave the variance alone
                assert mask_in == mask and mask_out not in (mask_in, NONE), case
                mask = mask_out
                mask_writes.append(mask_out)
        # the caller's buffers: the output once, by the last step; the input never; the mask and the variance once if wanted, else never
        assert image_writes.count(OUT) == 1 and image_writes[-1] == OUT and IN not in image_writes, case
        assert mask_writes.count(MC) == (1 if want_valid else 0) and (mask == MC) == want_valid, case
        wanted = with_var and want_var
        assert var_writes.count(VC) == (1 if wanted else 0) and (var == VC) == wanted, case
