"""The walker batteries of tests/walker_batteries.py through mi_render_rays: hand-built rays at the decision edges of the mesh traversal, in
every storage mode of the reference-tree walker (MI_RT_WF_TRAV_LDS = 0, 4, 5, 6: a context each), once more with the BVH in global memory
(MI_RT_GLOBAL_BVH = 1), under MI_OPT_REFERENCE_WALK, MI_OPT_TWO_STAGE and no flag.

Bars: the path signature of every table entry equals the oracle's orc_shade_sig on the stream (seed, y*W + x, 0) bit for bit — hit
distance bits, object index and RNG state of every segment; the f32 image lies within tests/test_gpu_ray_table.py's bars of orc_shade_sig's
colours; signatures and images are bit-identical across flags and modes; in the `one-emission` scene the colour of every entry whose
ray the census saw hit triangle k IS texel k + 33 of the index texture (no oracle involved).  Each scene is rendered four times: with
max_trace_dist far away, at a hit distance exactly and at its two f32 neighbours (kind d).  What the tables hold is counted on the CPU
(tests/test_walker_batteries_host.py)."""
import numpy as np
import pytest

from cs397raytracingsp22_amd import Scene, abi

import walker_batteries as wb
from test_gpu_ray_table import assert_within_bars
from test_gpu_walkers import context_with_env
from test_scene_compile_host import Blob, shim          # noqa: F401  (shim: fixture)

pytestmark = pytest.mark.gpu

MODES = {"0": {"MI_RT_WF_TRAV_LDS": 0}, "4": {"MI_RT_WF_TRAV_LDS": 4}, "5": {"MI_RT_WF_TRAV_LDS": 5}, "6": {"MI_RT_WF_TRAV_LDS": 6},
         "global-bvh": {"MI_RT_GLOBAL_BVH": 1}}
FLAGS = (abi.MI_OPT_REFERENCE_WALK, abi.MI_OPT_TWO_STAGE, 0)


@pytest.fixture(scope="module")
def bat(shim):                                          # noqa: F811
    sc, _, _ = wb.scene("one", 8)
    blob = Blob(shim, sc.flatten().desc)
    tree = wb.Tree(blob, 0)
    blob.close()
    return wb.battery(tree)


_REF, _FIRST = {}, {}


def reference(orc, sc, flat, key, o, d):
    """(f32 [H, W, 3], sig [H, W]) of orc_shade_sig per table entry; computed once per (scene, call) and left unchanged"""
    if key not in _REF:
        cam = sc.camera
        H, W = cam.screen_height, cam.screen_width
        osc = orc.OracleScene(flat)
        r32, rsig = np.zeros((H * W, 3), np.float32), np.zeros(H * W, np.uint32)
        for p in range(H * W):
            r32[p], rsig[p] = osc.shade_sig(cam, o[p], d[p], seed=wb.SEED, pixel=p, sample=0)
        osc.close()
        r32, rsig = r32.reshape(H, W, 3), rsig.reshape(H, W)
        r32.flags.writeable = rsig.flags.writeable = False
        _REF[key] = (r32, rsig)
    return _REF[key]


def render_and_compare(ctx, orc, sc, flat, key, o, d, what):
    """Every flag setting against the oracle and against each other; against the first mode that rendered this table."""
    cam = sc.camera
    H, W = cam.screen_height, cam.screen_width
    r32, rsig = reference(orc, sc, flat, key, o, d)
    to, td = o.reshape(H, W, 3), d.reshape(H, W, 3)
    base = None
    for flags in FLAGS:
        f32, _, sig, st = ctx.render_rays(cam, to, td, seed=wb.SEED, want_u8=False, want_sig=True, flags=flags)
        assert st.samples == W * H
        bad = np.flatnonzero(sig.ravel() != rsig.ravel())
        assert len(bad) == 0, f"{what}, flags {flags}: {len(bad)} of {W * H} entries took a different path than the oracle, the first {bad[:8]}"
        assert_within_bars(f32, None, r32, None, f"{what}, flags {flags}")
        base = base or (f32, sig)
        assert np.array_equal(f32.view(np.uint32), base[0].view(np.uint32)) and np.array_equal(sig, base[1]), (what, flags)
    first = _FIRST.setdefault(key, base)
    assert np.array_equal(base[0].view(np.uint32), first[0].view(np.uint32)) and np.array_equal(base[1], first[1]), f"{what}: differs from the first mode"
    return base


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", wb.SCENES)
def test_walker_battery(orc, bat, name, mode):
    sc, M, index = wb.scene(name, bat["height"])
    flat = sc.flatten()
    o, d = wb.to_world(M, bat["o"], bat["d"])
    with context_with_env(MODES[mode]) as ctx:
        ctx.upload(flat)
        for call, t_max in enumerate(bat["calls"]):
            sc.camera.max_trace_dist = t_max
            f32, sig = render_and_compare(ctx, orc, sc, flat, (name, call), o, d, f"{name}, mode {mode}, max_trace_dist {t_max!r}")
            if call == 0:
                assert len(np.unique(sig)) > 200
                if name == "one-emission":          # the colour names the triangle the census saw win
                    hit = np.flatnonzero(bat["winner"] >= 0)
                    tx, ty = np.array([wb.texel_of_triangle(int(k)) for k in bat["winner"][hit]]).T
                    want = np.stack([tx, ty, np.zeros_like(tx)], axis=1).astype(np.float32) / np.float32(255.0)
                    got = f32.reshape(-1, 3)[hit]
                    err = np.abs(got.astype(np.float64) - want)
                    print(f"one-emission, mode {mode}: {len(hit)} entries name their triangle, {len(np.unique(bat['winner'][hit]))} different triangles, max error {err.max():.2e}")
                    assert len(hit) >= 1000 and err.max() <= 2e-5            # the texels are k / 255: neighbours are 3.9e-3 apart
        sc.camera.max_trace_dist = wb.FAR


@pytest.mark.parametrize("mode", ["0", "4", "5", "6"])
def test_tables_with_one_and_with_no_entering_ray(orc, bat, mode):
    """Kind i, scene `one`: a class-B queue of one path, and an empty one.  At path_depth 1 the table without an entering ray is wf_main's
    result alone: bit for bit the render of the walls without the mesh."""
    sc, M, _ = wb.scene("one", 1)
    flat = sc.flatten()
    walls = Scene(sc.camera, sc.objects[:-1])
    with context_with_env(MODES[mode]) as ctx:
        for which in ("one enters", "none enters"):
            o, d = wb.to_world(M, *bat["small"][which])
            ctx.upload(flat)
            sc.camera.path_depth = 4
            render_and_compare(ctx, orc, sc, flat, ("small", which), o, d, f"{which}, mode {mode}")
            sc.camera.path_depth = 1
            f32, sig = render_and_compare(ctx, orc, sc, flat, ("small depth 1", which), o, d, f"{which}, depth 1, mode {mode}")
            print(f"{which}, mode {mode}, depth 1: {ctx.last_pipeline_counts()}, {ctx.last_pipeline_ms()}")
            if which == "none enters":
                ctx.upload(walls.flatten())
                g32, _, gsig, _ = ctx.render_rays(sc.camera, o.reshape(1, -1, 3), d.reshape(1, -1, 3), seed=wb.SEED, want_u8=False, want_sig=True)
                assert np.array_equal(g32.view(np.uint32), f32.view(np.uint32)) and np.array_equal(gsig, sig)
                assert (f32.sum(axis=-1) > 0).any()                 # some of these rays end on the ceiling light
