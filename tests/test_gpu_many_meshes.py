"""Scenes past the widths of the mesh masks: 24, 25, 31, 32, 33 and 40 StaticMeshes in Scene.objects.

The mesh word of a tile mask and WfArgs' trav_mask have 32 bits, the two-stage candidate header has room for 24 mesh indices
(kTwoStageMaxMeshes), EmitFlags.mesh_mask covers the live meshes below 32.  What depends on those widths — enter_next_mesh,
enter_next_mesh_f, enters_two_stage_root, wf_replay, launch_walker's `multi`, plan_walker's `m >= 32`, the planner's n_mesh > 32 and
ref_walk, the final-segment cull's any_mesh — is run here on both sides of each width, against the oracle: signatures bit for bit,
images within the parity bars (tests/test_gpu_parity.py), and every pipeline setting bit-identical to every other.

The scene is the one-light Cornell box with n small meshes on a grid in front of the camera: cubes of 12 triangles and one-triangle
meshes (the root is a leaf) in alternation, each with a Lambertian colour of its own, so a swapped mesh index shows in the image
and in the signature (which folds the object index).  64 x 48 at 4 spp, depth 4.  The builders and the oracle's side run without a
GPU (tests/test_many_meshes_host.py checks what the scenes compile to)."""
import numpy as np
import pytest

from cs397raytracingsp22_amd import ConvexVolume, Isotropic, Lambertian, Scene, StaticMesh, abi, cgmath, scenes

from test_gpu_edge_cases import tiny_mesh
from test_gpu_parity import RMS_TOL
from test_gpu_ray_queries import check_scene, oracle_hits, same_f32
from test_gpu_walkers import context_with_env
from test_oracle_kat import cube_mesh
from test_scene_compile_host import WALK_GLOBAL, WALK_PAIRED, Blob, shim                # noqa: F401  (shim: fixture)

gpu = pytest.mark.gpu

SIZES = (24, 25, 31, 32, 33, 40)
W, H, SPP, DEPTH = 64, 48, 4, 4
SEED = 7
GLOW = (3.0, 3.0, 3.0)
_CUBE, _TRI = cube_mesh(-0.25, 0.25), tiny_mesh(1)


def mesh_colour(k):
    return (0.15 + 0.7 * ((k * 37) % 41) / 40.0, 0.15 + 0.7 * ((k * 11) % 43) / 42.0, 0.15 + 0.7 * ((k * 23) % 47) / 46.0)


def mesh_is_cube(k):
    return k % 2 == 0


def grid_centre(k):
    return (-2.45 + 0.7 * (k % 8), 0.7 + 1.1 * (k // 8), 1.0 - 0.35 * (k % 3))


def grid_mesh(k, cube=None, emits=False, scale=1.0):
    """Mesh k of the grid: 8 columns, rows upwards, three depths; a cube (even k) turned about y by 17 k degrees, or one triangle (odd k), which faces the camera within 60 degrees."""
    cube = mesh_is_cube(k) if cube is None else cube
    at = grid_centre(k)
    turn = cgmath.from_angle_y(17.0 * k) if cube else cgmath.from_angle_y(6.0 * (k % 8) - 21.0)
    xf = cgmath.mul(cgmath.from_translation(at), turn, cgmath.from_scale(scale if cube else 0.6 * scale))
    mat = Lambertian(albedo=mesh_colour(k), emission=GLOW if emits else (0.0, 0.0, 0.0))
    return StaticMesh(_CUBE if cube else _TRI, mat, [None] * 5, xf)


def walls(lit=True):
    out = scenes.cornell_walls()
    if not lit:
        for t in out:
            if any(t.material.emission):
                t.material = Lambertian(albedo=t.material.albedo)
    return out


def many_meshes_scene(n, emitters=None, cubes=(), volume=False):
    """The one-light box + n grid meshes.  emitters: the meshes that emit INSTEAD of the ceiling light (None: the ceiling light).
    cubes: indices that are the cube whatever their parity.  volume: a ConvexVolume bounded by a cube StaticMesh, listed behind the grid, placed above and in front of it."""
    objs = walls(lit=emitters is None)
    glows = lambda k: emitters is not None and k in emitters                    # noqa: E731  (an emitter is 2.5 times the size: enough paths find it)
    objs += [grid_mesh(k, cube=True if k in cubes else None, emits=glows(k), scale=2.5 if glows(k) else 1.0) for k in range(n)]
    if volume:
        bound = StaticMesh(cube_mesh(-0.9, 0.9), Lambertian(albedo=(0.6, 0.6, 0.6)), [None] * 5,
                           cgmath.mul(cgmath.from_translation((0.3, 5.0, 1.6)), cgmath.from_angle_y(25.0)))
        objs.append(ConvexVolume(bound, Isotropic(albedo=(0.9, 0.7, 0.5)), 3.0))
    return Scene(scenes.cornell_camera(W, H, SPP, DEPTH), objs)


_ORACLE = {}


def oracle_render(orc, key, sc):
    """(flat, f32, u8, sig) of the oracle, once per scene, shared and left unchanged"""
    if key not in _ORACLE:
        flat = sc.flatten()
        r32, r8, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=SEED)
        for a in (r32, r8, rsig):
            a.flags.writeable = False
        _ORACLE[key] = (flat, r32, r8, rsig)
    return _ORACLE[key]


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """(f32, u8, sig) triples equal bit for bit"""
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def assert_bars(f32, u8, r32, r8, what):
    err = np.abs(f32.astype(np.float64) - r32.astype(np.float64))
    rms = [float(np.sqrt(np.mean(err[..., ch] ** 2))) for ch in range(3)]
    rel = float((err / np.maximum(1.0, np.abs(r32.astype(np.float64)))).max())
    print(f"{what}: rms {rms}, max relative diff {rel:.3e}")
    assert max(rms) <= RMS_TOL, (what, rms)
    assert rel <= 2e-5, (what, rel)
    assert int(np.abs(u8.astype(int) - r8.astype(int)).max()) <= 1, what


def assert_is_the_oracle(got, ref, what):
    f32, u8, sig = got
    _, r32, r8, rsig = ref
    bad = int((sig != rsig).sum())
    assert bad == 0, f"{what}: {bad}/{sig.size} pixels took a different path than the oracle"
    assert_bars(f32, u8, r32, r8, what)


def reference_mask(n):
    """The meshes the default pipeline walks with the reference walker, as WfArgs.trav_mask has them: none of these meshes has the
    1024 triangles of a default two-stage mesh, and the word has 32 bits."""
    return (1 << min(n, 32)) - 1


# ---------------------------------------------------------------------------------------------- every n: the wavefront pipeline
FLAGS = {"default": 0, "reference walk": abi.MI_OPT_REFERENCE_WALK, "two-stage": abi.MI_OPT_TWO_STAGE, "no tile masks": abi.MI_OPT_NO_TILE_MASKS}


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_wavefront_pipeline_equals_the_oracle(gpu_ctx, orc, shim, n):                       # noqa: F811
    sc = many_meshes_scene(n)
    ref = oracle_render(orc, n, sc)
    flat = ref[0]
    assert flat.desc.n_objects == 10 + n and len(np.unique(ref[3])) > W * H // 2
    gpu_ctx.upload(flat)
    base = None
    for name, flags in FLAGS.items():
        got = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True, flags=flags)[:3]
        with_sig = gpu_ctx.last_pipeline_counts()
        gpu_ctx.render(sc.camera, seed=SEED, flags=flags)
        print(f"n = {n}, {name}: counts with signatures {with_sig}, without {gpu_ctx.last_pipeline_counts()}")
        assert_is_the_oracle(got, ref, f"n = {n}, {name}")
        base = base or got
        assert same(got, base), name
    b = Blob(shim, flat.desc)
    fits = [mode for mode in (WALK_GLOBAL, WALK_PAIRED) if b.plan(reference_mask(n), mode)["form"] == mode]
    b.close()
    assert fits == [WALK_GLOBAL, WALK_PAIRED]            # 40 small trees are a few KB: both forms hold them (test_many_meshes_host.py)
    for mode in fits:
        with context_with_env({"MI_RT_WF_TRAV_LDS": mode}) as ctx:
            ctx.upload(flat)
            for flags in (0, abi.MI_OPT_REFERENCE_WALK):
                got = ctx.render(sc.camera, seed=SEED, want_sig=True, flags=flags)[:3]
                assert_is_the_oracle(got, ref, f"n = {n}, walker mode {mode}, flags {flags}")
                assert same(got, base), mode


# ---------------------------------------------------------------------------------------------- n >= 32: the other kernels
BIG = (32, 33, 40)


@gpu
@pytest.mark.parametrize("variant", [abi.MI_VARIANT_VOTED, abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_RECURSIVE], ids=["voted", "simple", "recursive"])
@pytest.mark.parametrize("n", BIG)
def test_megakernel_variants_equal_the_oracle(gpu_ctx, orc, n, variant):
    sc = many_meshes_scene(n)
    ref = oracle_render(orc, n, sc)
    gpu_ctx.upload(ref[0])
    got = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True, variant=variant)[:3]
    assert_is_the_oracle(got, ref, f"n = {n}, variant {variant}")
    if variant == abi.MI_VARIANT_RECURSIVE:             # nests the products as the reference does
        assert np.array_equal(bits(got[0]), bits(ref[1]))


def fan(sc, n, n_rays, seed):
    """A seeded fan from the eye: ray i aims at mesh i % n, up to 0.22 beside its centre (a cube is 0.5 wide: some rays pass between
    the meshes and end on the walls); directions not normalised, lengths over two decades."""
    rng = np.random.default_rng(seed)
    eye = np.asarray(sc.camera.eyepoint, np.float64)
    at = np.array([grid_centre(i % n) for i in range(n_rays)]) + rng.uniform(-0.22, 0.22, (n_rays, 3))
    d = (at - eye) * 10.0 ** rng.uniform(-1, 1, (n_rays, 1))
    return np.ascontiguousarray(np.broadcast_to(eye.astype(np.float32), d.shape)), np.ascontiguousarray(d, np.float32)


@gpu
@pytest.mark.parametrize("n", BIG)
def test_ray_queries_equal_the_oracle(gpu_ctx, orc, n):
    """mi_intersect_rays in its full form (check_scene: camera, bounce and edge rays, every field) and its visibility form;
    mi_occluded_rays and mi_shade_rays on a fan of 512 rays."""
    sc = many_meshes_scene(n)
    check_scene(gpu_ctx, orc, f"many-{n}", sc, named=False)                    # uploads
    flat = sc.flatten()
    osc = orc.OracleScene(flat)
    o, d = fan(sc, n, 512, n)
    ref = oracle_hits(osc, o, d, 0.001, float("inf"), SEED, 40)
    kinds = np.array([flat.desc.objects[k].kind for k in range(flat.desc.n_objects)])
    won = np.unique(ref["object"][ref["object"] >= 0])
    mesh_won = [int(k) - 10 for k in won if kinds[k] == abi.MI_OBJ_MESH]
    print(f"n = {n}: the fan's closest hits name {len(mesh_won)} of the {n} meshes, the last {max(mesh_won)}")
    walls_won = int((kinds[ref["object"]] != abi.MI_OBJ_MESH).sum())
    assert len(mesh_won) >= n - 3 and walls_won >= 64 and (n <= 32 or sum(k >= 32 for k in mesh_won) >= n - 33)      # the meshes past the mask are seen
    vis = gpu_ctx.intersect_rays(o, d, seed=SEED, first_key=40, resolve=False)
    assert vis.hitpoint is None and np.array_equal(vis.object, ref["object"]) and same_f32(vis.distance, ref["distance"])
    D = ref["distance"]
    for what, tm in (("inf", np.full(len(o), np.inf, np.float32)), ("at the hit", D), ("one ulp above", np.nextafter(D, np.float32(np.inf)))):
        tm = np.where(ref["object"] >= 0, tm, np.float32(np.inf)).astype(np.float32)
        want = np.array([bool(osc.intersect(o[i], d[i], t_min=0.001, t_max=float(tm[i]), seed=SEED, pixel=40 + i).hit) for i in range(len(o))])
        got = gpu_ctx.occluded_rays(o, d, ray_t_max=tm, seed=SEED, first_key=40)
        assert np.array_equal(got, want), (n, what, np.flatnonzero(got != want)[:8])
    shade = np.stack([osc.shade(sc.camera, o[i], d[i], seed=SEED, pixel=900 + i, sample=0) for i in range(len(o))])
    got = gpu_ctx.shade_rays(sc.camera, o, d, seed=SEED, first_key=900)
    osc.close()
    assert (shade.sum(axis=1) > 0).sum() >= 100
    assert same_f32(got, shade)


# ---------------------------------------------------------------------------------------------- the final-segment cull past bit 31
@gpu
@pytest.mark.parametrize("emitter", [32, 31])
def test_final_cull_with_the_only_emitter_at_the_mask_edge(gpu_ctx, orc, emitter):
    """33 meshes, one of them the scene's only emitter: mesh 32 has no bit in EmitFlags.mesh_mask and is known through any_mesh
    alone; mesh 31 has the last bit.  want_sig=False selects the SIG = false forms, the ones that cull."""
    sc = many_meshes_scene(33, emitters=(emitter,))
    ref = oracle_render(orc, ("emitter", emitter), sc)
    lit = int((ref[1].sum(axis=-1) > 0).sum())
    print(f"only emitter mesh {emitter}: {lit} lit pixels in the reference")
    assert lit >= 100
    gpu_ctx.upload(ref[0])
    f32, u8, none, _ = gpu_ctx.render(sc.camera, seed=SEED, want_sig=False)
    cull = gpu_ctx.last_pipeline_counts()
    g32, g8, _, _ = gpu_ctx.render(sc.camera, seed=SEED, want_sig=False, flags=abi.MI_OPT_NO_FINAL_CULL)
    print(f"only emitter mesh {emitter}: counts with the cull {cull}, without {gpu_ctx.last_pipeline_counts()}")
    assert none is None
    assert np.array_equal(bits(f32), bits(g32)) and np.array_equal(u8, g8)
    assert_bars(f32, u8, ref[1], ref[2], f"only emitter mesh {emitter}")
    s32, s8, sig, _ = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True)
    assert np.array_equal(sig, ref[3]) and np.array_equal(bits(s32), bits(f32))


# ---------------------------------------------------------------------------------------------- the two-stage index limit
def two_stage_limit_scene():
    """25 meshes of which 23 and 24 are both the cube: index 23 is the last the candidate header can name, 24 the first it cannot."""
    return many_meshes_scene(25, cubes=(23, 24))


@gpu
def test_two_stage_walk_at_the_index_limit(gpu_ctx, orc):
    sc = two_stage_limit_scene()
    ref = oracle_render(orc, "two-stage limit", sc)
    gpu_ctx.upload(ref[0])
    walk = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True, flags=abi.MI_OPT_REFERENCE_WALK)[:3]
    two = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True, flags=abi.MI_OPT_TWO_STAGE)[:3]
    ms = gpu_ctx.last_pipeline_ms()
    print(f"two-stage limit: {ms}")
    assert ms["wf_trav_f_ms"] > 0.0 and ms["wf_trav_ms"] > 0.0          # both walkers ran: meshes below 24 in two stages, mesh 24 by reference
    assert np.array_equal(two[2], ref[3]) and np.array_equal(walk[2], ref[3])
    assert np.array_equal(bits(two[0]), bits(walk[0])) and np.array_equal(two[1], walk[1])
    assert_bars(two[0], two[1], ref[1], ref[2], "two-stage limit")


# ---------------------------------------------------------------------------------------------- a boundary mesh past index 32
def volume_scene():
    return many_meshes_scene(32, volume=True)


@gpu
@pytest.mark.parametrize("flags", [0, abi.MI_OPT_REFERENCE_WALK, abi.MI_OPT_TWO_STAGE], ids=["default", "reference walk", "two-stage"])
def test_volume_boundary_record_past_the_listed_meshes(gpu_ctx, orc, flags):
    sc = volume_scene()
    ref = oracle_render(orc, "volume", sc)
    gpu_ctx.upload(ref[0])
    got = gpu_ctx.render(sc.camera, seed=SEED, want_sig=True, flags=flags)[:3]
    assert_is_the_oracle(got, ref, f"volume behind 32 meshes, flags {flags}")
