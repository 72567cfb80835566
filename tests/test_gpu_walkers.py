"""Every storage mode of the reference-tree walker gives the same paths: BVH in global memory (0), and wf_trav_i — interior nodes in
LDS, leaves from global memory, two 1024-thread blocks per CU (4: what trees of 64 .. 150 KB such as obj/drone.obj take by default),
with the leaf records in LDS too (5: trees whose whole split image fits 64 KB), or that with the interior records in the paired {near, far} layout (6: the default for SEVERAL small trees; one small tree - the
teapot - takes mode 5, whose single-mesh form tests boxes with the clamped v_med3 form).  The mode is a developer knob read once in
mi_ctx_create (MI_RT_WF_TRAV_LDS), so each mode gets a context of its own; signatures must equal the oracle's bit for bit."""
import contextlib
import json
import os

import numpy as np
import pytest

from cs397raytracingsp22_amd import Context, Lambertian, StaticMesh, abi, cgmath, scenes

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def context_with_env(env):
    """A context of its own created under the given developer knobs (read once in mi_ctx_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        ctx = Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield ctx
    finally:
        ctx.close()


def render_with_env(env, flat, cam, seed, flags=0, want_sig=True):
    with context_with_env(env) as ctx:
        ctx.upload(flat)
        f32, _, sig, _ = ctx.render(cam, seed=seed, want_sig=want_sig, flags=flags)
        return f32, sig


def render_with_mode(mode, flat, cam, seed):
    return render_with_env({"MI_RT_WF_TRAV_LDS": mode}, flat, cam, seed, flags=abi.MI_OPT_REFERENCE_WALK)


def test_walker_storage_modes_agree_with_the_oracle_teapot(orc):
    sc = scenes.config2(144, 96, 16, 10)
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=4)
    ref = None
    for mode in (0, 4, 5, 6):
        f32, sig = render_with_mode(mode, flat, sc.camera, 4)
        assert int((sig != rsig).sum()) == 0, f"walker mode {mode}: paths differ from the oracle"
        ref = f32 if ref is None else ref
        assert np.array_equal(f32, ref), mode


def test_walker_storage_modes_agree_several_meshes_and_a_leaf_root(orc):
    """Teapot + cube + a one-triangle mesh (its root is a leaf: never box-tested, geometry.rs:95) + the teapot again."""
    from test_oracle_kat import cube_mesh
    from test_gpu_edge_cases import tiny_mesh
    sc = scenes.config2(128, 96, 16, 8)
    grey = Lambertian(albedo=(0.7, 0.7, 0.7))
    sc.objects.append(StaticMesh(cube_mesh(-0.5, 0.5), grey, [None] * 5, cgmath.from_translation((-1.8, 0.5, 1.0))))
    sc.objects.append(StaticMesh(tiny_mesh(1), grey, [None] * 5, cgmath.from_translation((1.5, 2.5, 0.5))))
    sc.objects.append(sc.objects[-3])                                     # the teapot once more (shared StaticMesh)
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=11)
    for mode in (0, 4, 5, 6):
        _, sig = render_with_mode(mode, flat, sc.camera, 11)
        assert int((sig != rsig).sum()) == 0, f"walker mode {mode}: paths differ from the oracle"


def test_drone_takes_the_interior_in_lds_walker_and_matches(orc, gpu_ctx):
    """cfg4's tree (3471 nodes: 140 KB as a whole image, 55 KB of interior nodes) at a small size: default mode against mode 0."""
    sc = scenes.config4(96, 64, 16, 6, tex_size=64)
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=2)
    gpu_ctx.upload(flat)
    _, _, sig, _ = gpu_ctx.render(sc.camera, seed=2, want_sig=True)
    assert int((sig != rsig).sum()) == 0
    _, sig0 = render_with_mode(0, flat, sc.camera, 2)
    assert np.array_equal(sig0, rsig)


SCHEDULE_SCENES = {"cfg1": lambda: scenes.config1(160, 96, 16, 8), "cfg2": lambda: scenes.config2(160, 96, 16, 10),
                   "cfg5": lambda: scenes.config5(96, 64, 8, 50),
                   "head": lambda: scenes.head_scene(96, 96, 8, 10)}      # head: meshes of both kinds (reference walk + two-stage)


@pytest.mark.parametrize("scene", ["cfg1", "cfg2", "cfg5", "head"])
def test_pass_schedules_agree_with_the_oracle(orc, scene):
    """The pass-by-pass schedule (every pass through the HBM path state, one or two in-launch rounds), the tail schedule (a pass
    that no longer fills the chip runs every path as far as it can inside one launch — what frames this small take by default)
    and a schedule that waits for every header give the same paths."""
    sc = SCHEDULE_SCENES[scene]()
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=9)
    ref = None
    for env in ({"MI_RT_WF_TAIL_PATHS": 0}, {"MI_RT_WF_TAIL_PATHS": 4000}, {"MI_RT_WF_TAIL_PATHS": 1 << 22},
                {"MI_RT_WF_TAIL_PATHS": 0, "MI_RT_WF_NOWAIT_BLOCKS": 0}):
        f32, sig = render_with_env(env, flat, sc.camera, 9)
        assert int((sig != rsig).sum()) == 0, f"{env}: paths differ from the oracle"
        ref = f32 if ref is None else ref
        assert np.array_equal(f32, ref), env


def schedule_combos(scene):
    """{name: developer knobs} of the pinned schedules of one scene.  MI_RT_WF_NOWAIT_BLOCKS=0 in every one: only a host that
    waits for every header launches a schedule that does not depend on when the headers arrive (with run-ahead up to three
    surplus passes are launched, depending on timing: those runs are deliberately not pinned)."""
    out = {}
    for tail in (0, 4000, "unset"):
        for split in (0, "unset"):
            for conc in ((0, "unset") if scene == "head" else ("unset",)):      # head: the one scene with meshes of both kinds
                knobs = {"MI_RT_WF_TAIL_PATHS": tail, "MI_RT_WF_SPLIT": split, "MI_RT_WF_CONC": conc}
                name = f"tail_paths={tail} split={split}" + (f" conc={conc}" if scene == "head" else "")
                out[name] = dict({k: v for k, v in knobs.items() if v != "unset"}, MI_RT_WF_NOWAIT_BLOCKS=0)
    return out


def observe_schedule(scene, rounds):
    """{combination: launches, the eight pipeline counts, which kinds of launch happened} of SCHEDULE_SCENES[scene]; rounds = False:
    without the in-launch rounds of the passes before the tail (MI_RT_WF_FUSE_MIN=65: a wave has 64 lanes)."""
    sc = SCHEDULE_SCENES[scene]()
    flat = sc.flatten()
    out = {}
    for name, env in schedule_combos(scene).items():
        assert all(k not in os.environ for k in ("MI_RT_WF_TAIL_PATHS", "MI_RT_WF_SPLIT", "MI_RT_WF_CONC", "MI_RT_WF_FUSE_MIN")), "unset means unset"
        with context_with_env(env if rounds else dict(env, MI_RT_WF_FUSE_MIN=65)) as ctx:
            ctx.upload(flat)
            ctx.render(sc.camera, seed=9, want_sig=True)
            ms = ctx.last_pipeline_ms()
            out[name] = dict(ctx.last_pipeline_counts(), launches=ms.pop("launches"), kinds=sorted(k[:-3] for k, v in ms.items() if v > 0.0))
    return out


@pytest.mark.parametrize("scene", ["cfg1", "cfg2", "cfg5", "head"])
def test_pass_schedule_is_the_recorded_one(scene):
    """With every header waited for, the passes of a frame, their launches and their path counts follow from the scene and the
    scheduling knobs.  tests/golden/pass_schedule_counts.json holds them as the pass loop that made every scheduling decision inline
    in mi_rt.cpp launched them (recorded on an MI355X, eight frames per combination, before the decisions moved to render_plan.cpp's
    pass_schedule / pass_gate / plan_pass): tail never / mid-frame / from the first pass on, wf_main in one or two parts, and on the
    scene with meshes of both kinds wf_trav and wf_trav_f one after the other or side by side.

    Waiting for the headers is not enough to pin every number.  Whether a wave takes a further round inside a launch is a vote of
    its lanes, and which paths share a wave depends on the order of the previous pass' atomic appends: in the eight recorded frames
    of a combination with a pass before the tail, paths_a, paths_b and queue_entries took eight different values (cfg1, tail_paths=0:
    paths_a 138897 .. 139191), and cfg5 with tail_paths=4000 reached the tail after 30 or after 31 passes.  So every combination
    is rendered twice:
      "rounds"     as a frame is launched.  Pinned: which kinds of launch happened and the four counts no schedule can change
                   (sample_slots, pixels, segments, dead_tile_samples); with tail_paths unset, where every pass after the camera pass
                   is a tail pass and no vote is left, all eight counts and the launches (null in the file = not pinned).
      "no_rounds"  with MI_RT_WF_FUSE_MIN=65, which no wave of 64 lanes reaches: every pass before the tail moves every path by one
                   segment.  Pinned: all eight counts, the kinds and the launches.  On the head scene with tail_paths=0 and split
                   unset one late pass has its class-A blocks at the split threshold of 64 — the blocks are per shard, and the shard
                   of a path follows from the block that held it — and was launched in one part in some of the eight frames and in
                   two in the others: 65 or 66 launches, both recorded."""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pass_schedule_counts.json")) as fh:
        want = json.load(fh)[scene]
    got = {"rounds": observe_schedule(scene, True), "no_rounds": observe_schedule(scene, False)}
    assert sorted(want) == ["no_rounds", "rounds"]
    for mode in got:
        assert sorted(got[mode]) == sorted(want[mode])
        for name, seen in got[mode].items():
            print(scene, mode, name, seen)
            pinned = {k: v for k, v in want[mode][name].items() if v is not None}
            assert len(pinned) == 10 or (mode == "rounds" and "tail_paths=unset" not in name and len(pinned) == 5), (mode, name)
            for k, v in pinned.items():
                assert seen[k] in v if k == "launches" and isinstance(v, list) else seen[k] == v, (scene, mode, name, k, seen[k], v)


@pytest.mark.parametrize("mode", [0, 4, 5, 6])
def test_axis_aligned_rays_through_meshes(orc, mode):
    """Rays with exactly zero direction components: 1/d is infinite on two axes and the slab test meets NaN products (0 * inf) at
    box planes through the ray, which the reference's f32::max / min drop (geometry.rs:59-76).  An orthographic camera along -z
    sends every camera ray with d = (0, 0, -1) into meshes that are only translated, so object space sees the same direction; a
    mirror cube reflects some of them straight back.  (Written for an experimental v_med3 form of the walkers' box test, which
    needs another form for exactly these rays — tools/experiments/r03_walker_med3_slab.diff; kept as a parity case of its own.)"""
    from test_oracle_kat import cube_mesh
    from cs397raytracingsp22_amd import Metal
    sc = scenes.config2(96, 64, 8, 6)
    sc.camera.projection_mode = abi.MI_PROJ_ORTHOGRAPHIC
    sc.camera.view_dir = (0.0, 0.0, -1.0)
    grey = Lambertian(albedo=(0.7, 0.7, 0.7))
    sc.objects.append(StaticMesh(cube_mesh(-0.5, 0.5), grey, [None] * 5, cgmath.from_translation((0.0, 2.0, 0.5))))
    sc.objects.append(StaticMesh(cube_mesh(-0.25, 0.25), Metal(albedo=(0.9, 0.9, 0.9), roughness=0.0), [None] * 5, cgmath.from_translation((0.5, 2.0, 1.5))))
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=21)
    _, sig = render_with_mode(mode, flat, sc.camera, 21)
    assert int((sig != rsig).sum()) == 0, f"walker mode {mode}: paths differ from the oracle"


@pytest.mark.parametrize("mode", [4, 5, 6])
def test_axis_aligned_rays_through_one_mesh(orc, mode):
    """The same rays against ONE mesh: the single-mesh forms of wf_trav_i over 32-byte records (modes 4 and 5) test boxes with the clamped
    form (slab_med3) and must send a wave that holds a ray with a zero direction component through the reference form instead — here every
    camera ray is such a ray, and the mirror cube returns some of them along the axis.  Mode 6 (paired records) has no such split."""
    from test_oracle_kat import cube_mesh
    from cs397raytracingsp22_amd import Metal
    sc = scenes.config1(96, 64, 8, 6)                                      # the Cornell box without the teapot
    sc.camera.projection_mode = abi.MI_PROJ_ORTHOGRAPHIC
    sc.camera.view_dir = (0.0, 0.0, -1.0)
    sc.objects.append(StaticMesh(cube_mesh(-0.6, 0.6), Metal(albedo=(0.9, 0.9, 0.9), roughness=0.0), [None] * 5, cgmath.from_translation((0.25, 2.0, 0.5))))
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=23)
    _, sig = render_with_mode(mode, flat, sc.camera, 23)
    assert int((sig != rsig).sum()) == 0, f"walker mode {mode}: paths differ from the oracle"


def test_clamped_box_test_on_the_drone_with_grazing_and_axis_parallel_rays(orc):
    """cfg4's tree through its default walker (mode 4, one mesh: the clamped box test) under an orthographic camera along -x: every camera ray
    has two zero direction components (the reference form, rolled loop), the bounce rays have none (the clamped form) - both inside one render."""
    sc = scenes.config4(80, 56, 8, 6, tex_size=32)
    sc.camera.projection_mode = abi.MI_PROJ_ORTHOGRAPHIC
    sc.camera.view_dir = (-1.0, 0.0, 0.0)
    sc.camera.up = (0.0, 1.0, 0.0)
    flat = sc.flatten()
    _, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=5)
    f32, sig = render_with_env({}, flat, sc.camera, 5)
    assert int((sig != rsig).sum()) == 0
