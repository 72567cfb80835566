"""The wavefront pipeline's pass schedule, host side (CPU only): cs397raytracingsp22_amd/csrc/render_plan.cpp pass_schedule (what is
fixed for a render), pass_gate (may pass `it` be launched before the header of pass it - 1 has arrived?) and plan_pass (the grids, the
two parts, the tail and the in-launch rounds of one pass), asked through tests/cpp/render_plan_shim.cpp with a header in hand — no GPU
and no libmi_rt.so.  Every expected value is written out from the rules (256 threads per block, 256 shards, at most 3 passes ahead)."""
import ctypes as C
import os
import subprocess

import pytest

from cs397raytracingsp22_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs397raytracingsp22_amd", "csrc")
EXACT, BOUND, WAIT = 0, 1, 2
AUTO = 0xffffffff


class ScheduleQuery(C.Structure):          # tests/cpp/render_plan_shim.cpp
    _fields_ = ([("n_meshes", C.c_int32), ("qualifies", C.c_uint32), ("default_ts", C.c_uint32), ("flags", C.c_uint32),
                 ("have_masks", C.c_int32), ("ref_mask", C.c_uint32), ("ts_mask", C.c_uint32),
                 ("walker_bpc", C.c_uint32), ("n_cus", C.c_int32), ("path_depth", C.c_uint32)]
                + [(k, C.c_int32) for k in ("split", "conc", "conc_trav_bpc", "conc_travf_bpc", "travf_bpc")]
                + [(k, C.c_uint32) for k in ("tail_paths", "nowait_blocks", "fuse_max", "fuse_min")]
                + [("it", C.c_uint32), ("seen", C.c_uint32), ("exact", C.c_int32), ("n_in", C.c_uint32),
                   ("hdr_blocks", C.c_uint32), ("hdr_live", C.c_uint32), ("hdr_blocks_a", C.c_uint32)]
                + [("s_ref_mask", C.c_uint32), ("s_ts_mask", C.c_uint32)]
                + [(k, C.c_int32) for k in ("have_walkers", "ref_walk", "side_by_side", "split_enabled")]
                + [(k, C.c_uint32) for k in ("s_fuse_max", "s_fuse_min", "tail_fuse_max", "s_tail_paths", "s_nowait_blocks",
                                             "walker_blocks", "travf_blocks", "replay_blocks", "filter_blocks_per_shard")]
                + [("gate", C.c_int32), ("bound", C.c_uint32)]
                + [(k, C.c_int32) for k in ("stop", "p_split", "tail", "last")]
                + [(k, C.c_uint32) for k in ("grid_all", "grid_a", "grid_b", "p_fuse_max", "p_fuse_min")])


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    so = tmp_path_factory.mktemp("ps") / "render_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-shared",
                    os.path.join(CSRC, "render_plan.cpp"), os.path.join(CSRC, "scene_compile.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "render_plan_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.pass_schedule_defaults.argtypes = lib.pass_schedule_query.argtypes = [C.POINTER(ScheduleQuery)]
    lib.pass_schedule_defaults.restype = lib.pass_schedule_query.restype = None

    def ask(**kw):
        """The schedule, the gate and the plan for the given fields; knobs not given are the library's defaults, the device has 256
        CUs, the walker plan 2 blocks per CU and the camera path_depth 10."""
        q = ScheduleQuery(n_cus=256, walker_bpc=2, path_depth=10)
        lib.pass_schedule_defaults(C.byref(q))
        for k, v in kw.items():
            assert hasattr(q, k), k
            setattr(q, k, v)
        lib.pass_schedule_query(C.byref(q))
        return q
    return ask


NO_MESH = dict(n_meshes=0)
ONE_REF = dict(n_meshes=1)                                               # one mesh the two-stage bound does not apply to
ONE_TS = dict(n_meshes=1, qualifies=1, default_ts=1)
BOTH = dict(n_meshes=3, qualifies=0b100, default_ts=0b100)               # meshes 0, 1: reference walk; mesh 2: two-stage


def test_the_default_knobs(ask):
    q = ask()
    assert (q.split, q.conc, q.conc_trav_bpc, q.conc_travf_bpc, q.travf_bpc) == (1, 1, 0, 0, 0)
    assert (q.tail_paths, q.nowait_blocks, q.fuse_max, q.fuse_min) == (AUTO, 16384, 0, 32)


# ---------------------------------------------------------------------------------------------- the gate
def test_gate_runs_ahead_up_to_the_block_bound(ask):
    # 4 063 487 = 15872 * 256 + 255: 15872 full blocks + 2 * 256 partial ones = 16384, the default nowait_blocks exactly
    q = ask(it=2, seen=1, hdr_live=4063487)
    assert (q.bound, q.gate) == (16384, BOUND)
    q = ask(it=2, seen=1, hdr_live=4063488)
    assert (q.bound, q.gate) == (16385, WAIT)
    assert ask(it=2, seen=1, hdr_live=4063487, nowait_blocks=16383).gate == WAIT
    assert ask(it=2, seen=1, hdr_live=0).bound == 512


def test_gate_with_nowait_blocks_0_always_waits(ask):
    for live in (0, 1, 100000):
        assert ask(it=1, seen=0, hdr_live=live, nowait_blocks=0).gate == WAIT


def test_gate_runs_at_most_three_passes_ahead(ask):
    assert ask(it=5, seen=2, hdr_live=1000).gate == BOUND
    assert ask(it=6, seen=2, hdr_live=1000).gate == WAIT
    assert ask(it=4, seen=0, hdr_live=1000).gate == WAIT and ask(it=3, seen=0, hdr_live=1000).gate == BOUND


def test_gate_is_exact_when_every_header_has_been_read(ask):
    assert ask(it=0, seen=0, hdr_live=1 << 30).gate == EXACT
    assert ask(it=4, seen=4, hdr_live=1 << 30, nowait_blocks=0).gate == EXACT


# ---------------------------------------------------------------------------------------------- the plan: grids
@pytest.mark.parametrize("n_in, blocks", [(1, 1), (256, 1), (257, 2)])
def test_the_camera_pass_takes_its_grid_from_the_path_count(ask, n_in, blocks):
    for scene in (NO_MESH, ONE_REF):
        q = ask(it=0, exact=1, n_in=n_in, **scene)
        assert (q.grid_all, q.grid_a, q.stop, q.p_split) == (blocks, 0, 0, 0)


def test_an_exact_pass_takes_both_grids_from_the_header(ask):
    q = ask(it=3, exact=1, hdr_blocks=700, hdr_blocks_a=300, hdr_live=100000, **ONE_REF)
    assert (q.grid_all, q.grid_a, q.grid_b, q.stop) == (700, 300, 400, 0)


def test_a_pass_ahead_of_its_header_takes_the_upper_bound(ask):
    # 100 000 paths: 390 full blocks + 512; the header's own grids (of an older pass) are not used
    q = ask(it=3, exact=0, hdr_blocks=700, hdr_blocks_a=300, hdr_live=100000, **ONE_REF)
    assert (q.grid_all, q.grid_a, q.grid_b, q.stop) == (902, 902, 902, 0)


def test_an_empty_grid_stops(ask):
    assert ask(it=3, exact=1, hdr_blocks=0, hdr_blocks_a=0, hdr_live=0).stop == 1
    assert ask(it=3, exact=1, hdr_blocks=1, hdr_blocks_a=0, hdr_live=1).stop == 0
    assert ask(it=3, exact=0, hdr_live=0).stop == 0                      # the bound is never empty


# ---------------------------------------------------------------------------------------------- the plan: two parts
def test_split_needs_64_class_a_blocks_and_some_class_b_block(ask):
    hdr = dict(it=3, exact=1, hdr_blocks=700, hdr_live=100000)
    assert ask(hdr_blocks_a=63, **hdr, **ONE_REF).p_split == 0
    q = ask(hdr_blocks_a=64, **hdr, **ONE_REF)
    assert (q.p_split, q.grid_a, q.grid_b) == (1, 64, 636)
    assert ask(hdr_blocks_a=699, **hdr, **ONE_REF).p_split == 1
    assert ask(hdr_blocks_a=700, **hdr, **ONE_REF).p_split == 0           # grid_a == grid_all: no class-B block


def test_a_pass_ahead_of_its_header_is_split_when_there_are_walkers(ask):
    q = ask(it=3, exact=0, hdr_live=100000, **ONE_REF)
    assert (q.p_split, q.grid_a, q.grid_b) == (1, 902, 902)                # each part on the bound of the whole pass
    assert ask(it=3, exact=0, hdr_live=100000, **ONE_TS).p_split == 1
    assert ask(it=3, exact=0, hdr_live=100000, **NO_MESH).p_split == 0


def test_no_split_in_the_camera_pass_without_walkers_or_with_the_knob_off(ask):
    assert ask(it=0, exact=1, n_in=1 << 20, **ONE_REF).p_split == 0
    hdr = dict(it=3, exact=1, hdr_blocks=700, hdr_blocks_a=300, hdr_live=100000)
    assert ask(**hdr, **ONE_REF).p_split == 1
    assert ask(**hdr, **NO_MESH).p_split == 0
    assert ask(split=0, **hdr, **ONE_REF).p_split == 0
    assert ask(split=0, it=3, exact=0, hdr_live=100000, **ONE_REF).p_split == 0


# ---------------------------------------------------------------------------------------------- the plan: the tail
def test_tail_from_the_threshold_down(ask):
    for scene in (NO_MESH, ONE_REF):
        hdr = dict(it=2, exact=1, hdr_blocks=20, tail_paths=4000, **scene)
        assert ask(hdr_live=4000, **hdr).tail == 1
        assert ask(hdr_live=4001, **hdr).tail == 0
        assert ask(it=2, exact=0, hdr_live=4000, tail_paths=4000, **scene).tail == 1     # ahead of the header too


def test_the_camera_pass_is_never_a_tail_pass(ask):
    q = ask(it=0, exact=1, n_in=100, tail_paths=4000)
    assert (q.tail, q.last, q.p_fuse_max, q.p_fuse_min) == (0, 0, 2, 32)


def test_tail_knob_0_is_never(ask):
    for live in (0, 1, 4000):
        q = ask(it=2, exact=1, hdr_blocks=1, hdr_live=live, tail_paths=0)
        assert (q.s_tail_paths, q.tail, q.last) == (0, 0, 0)


def test_the_automatic_tail_threshold(ask):
    assert ask(**NO_MESH).s_tail_paths == 4 << 20
    for scene in (ONE_REF, ONE_TS, BOTH):
        assert ask(**scene).s_tail_paths == 1 << 20
    assert ask(tail_paths=4000, **ONE_REF).s_tail_paths == 4000
    hdr = dict(it=1, exact=1, hdr_blocks=5000)
    assert ask(hdr_live=1 << 20, **hdr, **ONE_REF).tail == 1 and ask(hdr_live=(1 << 20) + 1, **hdr, **ONE_REF).tail == 0
    assert ask(hdr_live=4 << 20, **hdr, **NO_MESH).tail == 1 and ask(hdr_live=(4 << 20) + 1, **hdr, **NO_MESH).tail == 0


def test_a_tail_pass_runs_every_path_as_far_as_it_can(ask):
    hdr = dict(it=2, exact=1, hdr_blocks=20, tail_paths=4000)
    for scene, normal_rounds in ((NO_MESH, 2), (ONE_REF, 1)):
        q = ask(hdr_live=4000, path_depth=10, **hdr, **scene)
        assert (q.tail_fuse_max, q.p_fuse_max, q.p_fuse_min) == (12, 12, 1)
        q = ask(hdr_live=4000, path_depth=50, fuse_min=7, **hdr, **scene)
        assert (q.p_fuse_max, q.p_fuse_min) == (52, 1)
        q = ask(hdr_live=4001, path_depth=50, fuse_min=7, **hdr, **scene)
        assert (q.p_fuse_max, q.p_fuse_min) == (normal_rounds, 7)


def test_a_tail_launch_is_the_last_only_without_walkers(ask):
    hdr = dict(it=2, exact=1, hdr_blocks=20, tail_paths=4000)
    assert ask(hdr_live=4000, **hdr, **NO_MESH).last == 1
    assert ask(hdr_live=4001, **hdr, **NO_MESH).last == 0
    for scene in (ONE_REF, ONE_TS, BOTH):
        q = ask(hdr_live=4000, **hdr, **scene)
        assert (q.tail, q.last) == (1, 0)


# ---------------------------------------------------------------------------------------------- the schedule of a render
def flags_of(q):
    return (q.have_walkers, q.ref_walk, q.side_by_side, q.split_enabled)


def test_schedule_of_a_scene_without_meshes(ask):
    q = ask(**NO_MESH)
    assert (q.s_ref_mask, q.s_ts_mask) == (0, 0) and flags_of(q) == (0, 0, 0, 0)
    assert (q.s_fuse_max, q.s_fuse_min, q.s_nowait_blocks) == (2, 32, 16384)
    q = ask(fuse_max=5, fuse_min=0, nowait_blocks=77, **NO_MESH)
    assert (q.s_fuse_max, q.s_fuse_min, q.s_nowait_blocks) == (5, 1, 77)     # fuse_min is at least 1


def test_schedule_with_reference_walk_meshes_only(ask):
    q = ask(n_meshes=2)
    assert (q.s_ref_mask, q.s_ts_mask) == (0b11, 0) and flags_of(q) == (1, 1, 0, 1)
    assert q.s_fuse_max == 1
    q = ask(flags=abi.MI_OPT_REFERENCE_WALK, **BOTH)                      # the flag sends every mesh through the reference walk
    assert (q.s_ref_mask, q.s_ts_mask) == (0b111, 0) and flags_of(q) == (1, 1, 0, 1)
    assert flags_of(ask(n_meshes=2, split=0)) == (1, 1, 0, 0)


def test_schedule_with_two_stage_meshes_only(ask):
    q = ask(n_meshes=2, qualifies=0b11, default_ts=0b11)
    assert (q.s_ref_mask, q.s_ts_mask) == (0, 0b11) and flags_of(q) == (1, 0, 0, 1)
    assert q.s_fuse_max == 1
    q = ask(n_meshes=2, qualifies=0b11, default_ts=0, flags=abi.MI_OPT_TWO_STAGE)      # the flag: every mesh the bound applies to
    assert (q.s_ref_mask, q.s_ts_mask) == (0, 0b11) and flags_of(q) == (1, 0, 0, 1)


def test_schedule_with_meshes_of_both_kinds(ask):
    q = ask(**BOTH)
    assert (q.s_ref_mask, q.s_ts_mask) == (0b011, 0b100) and flags_of(q) == (1, 1, 1, 1)
    q = ask(conc=0, **BOTH)
    assert (q.s_ref_mask, q.s_ts_mask) == (0b011, 0b100) and flags_of(q) == (1, 1, 0, 1)
    q = ask(n_meshes=3, qualifies=0b110, default_ts=0b100, flags=abi.MI_OPT_TWO_STAGE)
    assert (q.s_ref_mask, q.s_ts_mask) == (0b001, 0b110) and flags_of(q) == (1, 1, 1, 1)


def test_meshes_beyond_the_mask_bits_take_the_reference_walk(ask):
    q = ask(n_meshes=33, have_masks=1, ref_mask=0, ts_mask=0)            # 33 meshes, both masks empty: mesh 32 has no bit
    assert (q.s_ref_mask, q.s_ts_mask) == (0, 0) and flags_of(q) == (1, 1, 0, 1)
    assert q.s_tail_paths == 1 << 20 and q.s_fuse_max == 1
    q = ask(n_meshes=32, have_masks=1, ref_mask=0, ts_mask=0)            # (32 meshes all have one)
    assert flags_of(q) == (0, 0, 0, 0)
    q = ask(n_meshes=33)                                                  # as walk_masks gives them: every bit a reference walk
    assert (q.s_ref_mask, q.s_ts_mask) == (0xffffffff, 0) and flags_of(q) == (1, 1, 0, 1)
    q = ask(n_meshes=33, have_masks=1, ref_mask=0, ts_mask=0b1)
    assert flags_of(q) == (1, 1, 1, 1)


def test_block_counts(ask):
    dev = dict(n_cus=200, walker_bpc=3)
    q = ask(**dev, **ONE_REF)
    assert (q.walker_blocks, q.travf_blocks, q.replay_blocks, q.filter_blocks_per_shard) == (600, 1200, 1600, 8)
    q = ask(travf_bpc=4, **dev, **ONE_TS)
    assert (q.walker_blocks, q.travf_blocks, q.replay_blocks, q.filter_blocks_per_shard) == (600, 800, 1600, 8)
    # one after the other: the side-by-side overrides are not used
    for scene in (ONE_REF, ONE_TS, dict(conc=0, **BOTH)):
        q = ask(conc_trav_bpc=5, conc_travf_bpc=2, **dev, **scene)
        assert (q.walker_blocks, q.travf_blocks) == (600, 1200)
    assert ask(n_cus=304, walker_bpc=2, **ONE_REF).walker_blocks == 608


def test_block_counts_side_by_side(ask):
    dev = dict(n_cus=200, walker_bpc=3)
    q = ask(**dev, **BOTH)
    assert (q.walker_blocks, q.travf_blocks, q.replay_blocks, q.filter_blocks_per_shard) == (600, 1200, 1600, 8)
    assert ask(conc_trav_bpc=5, **dev, **BOTH).walker_blocks == 1000
    assert ask(conc_travf_bpc=2, **dev, **BOTH).travf_blocks == 400
    q = ask(travf_bpc=4, **dev, **BOTH)                                   # the side-by-side default follows the resolved travf_bpc
    assert (q.walker_blocks, q.travf_blocks) == (600, 800)
    q = ask(travf_bpc=4, conc_travf_bpc=2, conc_trav_bpc=1, **dev, **BOTH)
    assert (q.walker_blocks, q.travf_blocks) == (200, 400)
