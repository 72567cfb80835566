"""wf_main's final-segment cull (SIG = false forms) against the render without it, the signature render and the oracle.

A ray traced at level path_depth - 1 can only add the emission of its closest hit.  With signatures off, such a ray whose closest
list hit is a miss or cannot emit, and which entered no mesh root (or no mesh of the scene may emit), ends its path at once.  The
scenes also hold what a test order "emitters first" would have to get right (an emitter behind an occluder, a list of more than 64
entries, a medium that draws random numbers): that order was measured and left out, the cases stay.  The claim is "same image,
bit for bit", so every case renders three times —

    want_sig=False                               the cull
    want_sig=False, MI_OPT_NO_FINAL_CULL         the same kernels without it
    want_sig=True                                the SIG forms, which never had it

— and requires np.array_equal of the f32 and the u8 images (and equal bit patterns of the f32 where everything is finite; where
non-finite values are expected: equal_nan and equal NaN masks).  Every case also goes against the CPU oracle with the bars of
tests/test_gpu_signature_free.py (signatures bit-exact, RMS <= 1e-3, max rel err <= 2e-5, u8 <= 1 LSB, equal sign bits), and
over a whole frame segments + dead_tile_samples must equal the oracle's segment count with and without the cull: a culled
segment is still a segment."""
import ctypes as C

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Camera, Context, ConvexVolume, Dielectric, Isotropic, Lambertian, Metal, MultiContext, Plane, Scene,
                                     Sphere, StaticMesh, Texture, Triangle, abi, cgmath, scenes)
from cs397raytracingsp22_amd import dist as pdist

from test_gpu_signature_free import GREY, LIGHT, _bars, _cam, builds_top_tree, check_signature_free
from test_oracle_kat import cube_mesh

pytestmark = pytest.mark.gpu

NO_CULL = abi.MI_OPT_NO_FINAL_CULL


def bits(a):
    return a.view(np.uint32)


def paths(c):
    return c["paths_a"] + c["paths_b"]


def three_renders(ctx, cam, seed, flags=0, **kw):
    """(cull, no cull, signature render) as (f32, u8) pairs, and the pipeline counts of the first two"""
    f32, u8, sig, _ = ctx.render(cam, seed=seed, want_sig=True, flags=flags, **kw)
    g32, g8, none, _ = ctx.render(cam, seed=seed, flags=flags, **kw)
    c_cull = ctx.last_pipeline_counts()
    h32, h8, _, _ = ctx.render(cam, seed=seed, flags=flags | NO_CULL, **kw)
    c_plain = ctx.last_pipeline_counts()
    assert none is None
    return (g32, g8), (h32, h8), (f32, u8), c_cull, c_plain


def check_cull(ctx, orc, sc, seed, what, **kw):
    """check_signature_free (the cull against the signature render and the oracle, segment count included), then the three
    renders against each other.  Returns the counts with and without the cull."""
    check_signature_free(ctx, orc, sc, seed, **kw)
    (g32, g8), (h32, h8), (f32, u8), c_cull, c_plain = three_renders(ctx, sc.camera, seed, **kw)
    assert np.isfinite(f32).all(), what
    for name, (a32, a8) in (("cull", (g32, g8)), ("no cull", (h32, h8))):
        assert np.array_equal(a32, f32) and np.array_equal(a8, u8), (what, name)
        assert np.array_equal(bits(a32), bits(f32)), (what, name)
    # a culled segment is counted: the same segments.  (The paths streamed through HBM may go either way: fewer lanes end a pass with a
    # known hit, so fewer waves vote for a further round inside the launch and the emitter hits of a thin wave stream once more.)
    assert c_cull["segments"] == c_plain["segments"] and c_cull["dead_tile_samples"] == c_plain["dead_tile_samples"], (what, c_cull, c_plain)
    assert c_cull["queue_entries"] == c_cull["paths_b"] and c_plain["queue_entries"] == c_plain["paths_b"]
    print(f"{what}: paths through HBM {paths(c_plain)} -> {paths(c_cull)}, class B {c_plain['paths_b']} -> {c_cull['paths_b']}, "
          f"segments {c_cull['segments']}")
    return c_cull, c_plain


# ------------------------------------------------------------------------------------------------------- 1. the benchmarked scene
@pytest.mark.parametrize("depth", [1, 2, 3, 10])
def test_cfg2(gpu_ctx, orc, depth):
    """depth 1: the camera ray is the final segment, so the cull meets the tile masks in the camera pass."""
    sc = scenes.config2(96, 64, 8, depth)
    c_cull, c_plain = check_cull(gpu_ctx, orc, sc, 1, f"cfg2 depth {depth}")
    assert paths(c_cull) < paths(c_plain)                                # five of the box's six faces cannot emit
    if depth == 1:
        base, _, _, _ = gpu_ctx.render(sc.camera, seed=1)
        for flags in (abi.MI_OPT_NO_TILE_MASKS, abi.MI_OPT_NO_TILE_MASKS | NO_CULL):
            f32, _, _, _ = gpu_ctx.render(sc.camera, seed=1, flags=flags)
            assert np.array_equal(bits(f32), bits(base)), flags


# ------------------------------------------------------------------------------------- 2. emitters and occluders of every kind
def _near_cam(depth):
    """96 x 64, 8 spp, close enough for the objects around (0, 1, 0) to fill the frame"""
    return _cam(w=96, h=64, spp=8, depth=depth, eyepoint=(0.0, 1.3, 3.4), view_dir=(0.0, -0.12, -1.0))


def _floor(mat=GREY, wall=GREY):
    """a floor and a back wall, two Triangles each: most rays hit something that cannot emit"""
    return [Triangle((-4.0, 0.0, 3.4), (4.0, 0.0, 3.4), (4.0, 0.0, -3.0), mat), Triangle((-4.0, 0.0, 3.4), (4.0, 0.0, -3.0), (-4.0, 0.0, -3.0), mat),
            Triangle((-4.0, 0.0, -3.0), (4.0, 0.0, -3.0), (4.0, 5.0, -3.0), wall), Triangle((-4.0, 0.0, -3.0), (4.0, 5.0, -3.0), (-4.0, 5.0, -3.0), wall)]


def _small_teapot(at, material=None):
    material = material or Lambertian(albedo=(0.6, 0.3, 0.2))
    return StaticMesh(scenes.load_asset_mesh("teapot"), material, [None] * 5, cgmath.mul(cgmath.from_translation(at), cgmath.from_scale(0.25)))


def _emission_map():
    img = np.zeros((8, 8, 3), np.uint8)
    img[::2, 1::3] = (255, 160, 40)
    img[5, 5] = (0, 0, 1)                                                # the faintest texel that is not black
    return Texture(img)


def emitter_scene(kind, depth):
    cam = _near_cam(depth)
    if kind == "sphere":        # an emissive Sphere behind a plain Sphere and behind the teapot: the closest emitter is not the closest hit
        objs = _floor() + [Sphere((0.0, 1.1, -1.5), 0.9, LIGHT), Sphere((-0.55, 0.9, 0.4), 0.4, GREY),
                           Sphere((-1.6, 0.6, 0.0), 0.5, Metal(albedo=(0.8, 0.8, 0.8), roughness=0.1)), _small_teapot((0.45, 0.5, 0.9))]
    elif kind == "mesh":        # an emissive cube mesh (fixed material) beside a plain one: entering ANY root keeps the ray (the walker decides)
        objs = _floor() + [StaticMesh(cube_mesh(-0.5, 0.5), LIGHT, [None] * 5, cgmath.from_translation((-0.7, 0.9, 0.0))),
                           StaticMesh(cube_mesh(-0.35, 0.35), GREY, [None] * 5, cgmath.mul(cgmath.from_translation((0.7, 0.9, 0.3)), cgmath.from_angle_y(30.0))),
                           Sphere((0.0, 0.4, 1.0), 0.35, GREY)]
    elif kind == "map":         # a mesh that emits only through its emission map: the MESH = 2 forms
        green = scenes.load_asset_textures()["green"]
        objs = _floor() + [StaticMesh(cube_mesh(-0.7, 0.7), None, [green, _emission_map(), None, None, None],
                                      cgmath.mul(cgmath.from_translation((0.0, 0.9, 0.0)), cgmath.from_angle_y(35.0))),
                           Sphere((-1.1, 0.5, 0.6), 0.45, GREY), Sphere((1.1, 0.5, 0.6), 0.45, Dielectric(1.5))]
    elif kind == "volume":      # an emissive Isotropic medium: a hit that may emit and draws a random number
        objs = _floor() + [ConvexVolume(Sphere((0.0, 1.0, 0.0), 0.8, GREY), Isotropic(albedo=(0.9, 0.8, 0.7), emission=(0.5, 0.4, 0.3)), 1.5),
                           Sphere((-1.3, 0.5, 0.6), 0.45, GREY), Sphere((1.2, 0.5, 0.8), 0.4, Metal(albedo=(0.8, 0.7, 0.6), roughness=0.3))]
    elif kind == "dark_volume":  # a medium that cannot emit in front of an emissive Sphere
        objs = _floor() + [ConvexVolume(Sphere((0.0, 1.0, 0.6), 0.6, LIGHT), Isotropic(albedo=(0.9, 0.8, 0.7)), 1.5),
                           Sphere((0.0, 1.2, -1.2), 0.8, LIGHT), Sphere((-1.3, 0.5, 0.6), 0.45, GREY)]
    else:                       # an emissive Plane under plain objects: a Plane is never masked
        objs = [Plane((0.0, -0.2, 0.0), (0.0, 1.0, 0.0), Lambertian(albedo=(0.4, 0.4, 0.4), emission=(0.3, 0.25, 0.2))),
                Sphere((-0.7, 0.6, 0.0), 0.6, GREY), Sphere((0.8, 0.5, 0.5), 0.5, Metal(albedo=(0.8, 0.8, 0.8), roughness=0.2)),
                Triangle((-1.5, 0.0, -1.5), (1.5, 0.0, -1.5), (0.0, 2.4, -1.8), GREY)]
    return Scene(cam, objs)


EMITTERS = [(k, d) for k in ("sphere", "mesh", "map", "volume", "dark_volume", "plane") for d in (1, 2, 3)]


@pytest.mark.parametrize("kind,depth", EMITTERS, ids=[f"{k}-d{d}" for k, d in EMITTERS])
def test_emitters_and_occluders(gpu_ctx, orc, kind, depth):
    sc = emitter_scene(kind, depth)
    c_cull, c_plain = check_cull(gpu_ctx, orc, sc, 7, f"{kind} depth {depth}")
    r32, _, _, _ = orc.OracleScene(sc.flatten()).render(sc.camera, seed=7, want_u8=False, want_sig=False)
    assert int((r32.sum(axis=-1) > 0).sum()) >= 100                      # the emitter is in view: the case is not a black frame


# ----------------------------------------------------------------------------------------------- 3. non-finite throughput
def overflow_scene(depth=5):
    """Walls whose albedo makes T overflow at the second bounce (T = albedo 2 cos per bounce: 1e30 twice is past 3.4e38 for every
    cos above 1e-22), beside ordinary ones and an open front: at the last level some rays carry T = inf — 0 inf = NaN when they hit a
    non-emitter, nothing when they miss, so they must take the ordinary route — and others a finite T."""
    huge = Lambertian(albedo=(1e30, 1e30, 1e30))
    objs = _floor(huge, GREY) + [Sphere((0.0, 2.4, -0.5), 0.6, LIGHT), Sphere((-1.2, 0.6, 0.3), 0.6, GREY), Sphere((1.2, 0.6, 0.6), 0.6, huge)]
    return Scene(_near_cam(depth), objs)


def test_non_finite_throughput(gpu_ctx, orc):
    """The three renders agree, NaN masks included, and contain NaN pixels: a T = inf ray that hit a non-emitter at the last level.

    Against the oracle: the kernels carry a path as (L, T) and add T e at every hit; the reference — and the oracle — recurse,
    e + w (e' + w' (...)), where every w is finite.  Below the overflow the two agree within the bars; past it they cannot: 0 inf is a
    NaN in the first form and the second never forms that product (and would make an infinity only from a product of finite numbers).
    That holds for the SIG forms and without the cull alike.  So, beside the bit-exact signatures and the segment count over all pixels:
    every pixel the oracle makes non-finite is non-finite in the render, and the bars hold over the pixels the render keeps finite."""
    sc = overflow_scene()
    flat = sc.flatten()
    r32, r8, rsig, cnt = orc.OracleScene(flat).render(sc.camera, seed=9, want_counters=True)
    bad = ~np.isfinite(r32)
    assert bad.any() and (~bad.any(axis=-1) & (r32.sum(axis=-1) > 0)).any(), "the case needs non-finite pixels beside lit finite ones"
    gpu_ctx.upload(flat)
    (g32, g8), (h32, h8), (f32, u8), c_cull, c_plain = three_renders(gpu_ctx, sc.camera, 9)
    _, _, sig, _ = gpu_ctx.render(sc.camera, seed=9, want_sig=True)
    assert int((sig != rsig).sum()) == 0
    nan, inf = np.isnan(f32), np.isinf(f32)
    print(f"overflow: oracle {int(bad.any(axis=-1).sum())} non-finite pixels; render {int(nan.any(axis=-1).sum())} NaN, "
          f"{int(inf.any(axis=-1).sum())} inf pixels of {f32.shape[0] * f32.shape[1]}")
    assert nan.any(), "no T = inf ray met a non-emitter: the case tests nothing"
    for name, (a32, a8) in (("cull", (g32, g8)), ("no cull", (h32, h8))):
        assert np.array_equal(np.isnan(a32), nan) and np.array_equal(np.isinf(a32), inf), name
        assert np.array_equal(a32, f32, equal_nan=True) and np.array_equal(a8, u8), name
        assert np.array_equal(bits(a32)[~nan], bits(f32)[~nan]), name
    assert not np.isfinite(f32[bad]).any()
    keep = np.isfinite(f32).all(axis=-1)
    assert keep.sum() > keep.size // 2
    # pixels of ordinary radiance: the bars as they are.  A pixel that saw the light over ONE bounce off a 1e30 wall is finite and of
    # the order of 1e30, where the absolute RMS bar means nothing: there the relative bar alone, against the value itself
    plain = keep & (np.abs(r32).max(axis=-1) <= 1e3)
    assert plain.sum() > keep.size // 2 and (keep & ~plain).any()
    _bars(f32[plain], u8[plain], r32[plain], r8[plain], "overflow, finite pixels")
    big = keep & ~plain
    rel = np.abs(f32[big].astype(np.float64) - r32[big]) / np.maximum(1.0, np.abs(r32[big].astype(np.float64)))
    assert float(rel.max()) <= 2e-5, float(rel.max())
    assert int(np.abs(u8[big].astype(int) - r8[big].astype(int)).max()) <= 1
    for c in (c_cull, c_plain):
        assert c["segments"] + c["dead_tile_samples"] == cnt["segments"], (c, cnt["segments"])


# --------------------------------------------------------------------------------------------------------- 4. long lists
def long_list_scene(n_small, depth):
    """A floor and a wall, `n_small` small Triangles of which ONE emits (larger than the others, but within the 32 x median of the tree's
    rule), two spheres: more than 64 list entries (no 64-bit list mask covers them), and from 96 small Triangles on
    the TOP forms."""
    rng = np.random.default_rng(n_small)
    objs = _floor()
    for k in range(n_small):
        c = rng.uniform((-1.4, 0.2, -1.4), (1.4, 2.4, 0.8))
        lit = k == n_small // 2
        p = (0.3, 1.3, 0.6) + np.float64([(-0.45, -0.3, 0.0), (0.45, -0.3, 0.1), (0.0, 0.4, -0.1)]) if lit else c + rng.uniform(-0.14, 0.14, (3, 3))
        mat = LIGHT if lit else Lambertian(albedo=tuple(map(float, rng.uniform(0.3, 0.8, 3))))
        objs.append(Triangle(*[tuple(map(float, q)) for q in p], mat))
    objs += [Sphere((0.0, 0.5, 0.9), 0.4, Metal(albedo=(0.8, 0.8, 0.8), roughness=0.1)), Sphere((0.9, 0.4, 0.6), 0.35, GREY)]
    return Scene(_near_cam(depth), objs)


@pytest.mark.parametrize("n_small,depth", [(70, 1), (70, 3), (100, 1), (100, 3)], ids=["flat-d1", "flat-d3", "top-d1", "top-d3"])
def test_long_lists(gpu_ctx, orc, n_small, depth):
    sc = long_list_scene(n_small, depth)
    assert builds_top_tree(sc) == (n_small >= 96)
    assert sum(not isinstance(o, StaticMesh) for o in sc.objects) > 64
    c_cull, c_plain = check_cull(gpu_ctx, orc, sc, 13, f"{n_small} small triangles depth {depth}")
    assert paths(c_cull) != paths(c_plain)                               # rule 2 alone
    if n_small >= 96:                                                    # every Triangle one by one: the TOP = false form on a list of > 64 entries
        base, _, _, _ = gpu_ctx.render(sc.camera, seed=13)
        for flags in (abi.MI_OPT_NO_LIST_TREE, abi.MI_OPT_NO_LIST_TREE | NO_CULL):
            f32, _, _, _ = gpu_ctx.render(sc.camera, seed=13, flags=flags)
            assert np.array_equal(bits(f32), bits(base)), flags


# -------------------------------------------------------------------------------------- 5. batches, ranks, ray and point tables
def test_several_batches(gpu_ctx):
    sc = scenes.config2(96, 64, 9, 3)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    ref32, ref8, _, _ = gpu_ctx.render(sc.camera, seed=11, want_sig=True)
    one_batch = gpu_ctx.last_pipeline_ms()["launches"]
    npix = pdist.tiles_padded(sc.camera.screen_width, sc.camera.screen_height, 1) * pdist.TILE_PIXELS
    budget = npix * 4 * (2 * 6 * 16 + 16)                                # 4 + 4 + 1 samples
    small = Context(0)
    try:
        small.upload(flat)
        for flags in (0, NO_CULL):
            f32, u8, _, _ = small.render(sc.camera, seed=11, flags=flags, max_state_bytes=budget)
            assert small.last_pipeline_ms()["launches"] > one_batch
            assert np.array_equal(bits(f32), bits(ref32)) and np.array_equal(u8, ref8), flags
    finally:
        small.close()


def test_two_loopback_ranks():
    sc = scenes.config2(96, 64, 8, 2)
    flat = sc.flatten()
    one = Context(0)
    try:
        one.upload(flat)
        ref32, ref8, _, _ = one.render(sc.camera, seed=3, want_sig=True)
    finally:
        one.close()
    m = MultiContext.loopback(2)
    try:
        m.upload(flat)
        for flags in (0, NO_CULL):
            f32, u8, sig, _ = m.render(sc.camera, seed=3, want_sig=False, flags=flags)
            assert sig is None
            assert np.array_equal(bits(f32), bits(ref32)) and np.array_equal(u8, ref8), flags
    finally:
        m.close()


def test_ray_table_at_depth_one(gpu_ctx, orc):
    import test_gpu_ray_table as rt
    sc = rt._sized(scenes.config2(), 4, 1)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    o, d = rt.fan_table(sc.camera, 4, 21)
    f32, u8, _, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=rt.SEED, want_sig=True)
    for flags in (0, NO_CULL):
        g32, g8, _, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=rt.SEED, flags=flags)
        assert np.array_equal(bits(g32), bits(f32)) and np.array_equal(g8, u8), flags
    r32, r8 = rt.oracle_image(orc, flat, sc.camera, o, d, rt.SEED)
    assert int((r32.sum(axis=-1) > 0).sum()) >= 100                      # the ceiling is in view
    rt.assert_within_bars(f32, u8, r32, r8, "ray table depth 1")


def test_point_table_at_depth_one(gpu_ctx, orc):
    import test_gpu_point_table as pt
    import test_gpu_ray_table as rt
    sc = rt._sized(scenes.config2(), 4, 1)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    p, n = pt.point_table(orc, "config2", 1)                             # depth plays no part in the table or in the directions
    dirs = pt.directions(orc, "config2", 1)
    f32, u8, _, _ = gpu_ctx.render_points(sc.camera, p, n, seed=rt.SEED, want_sig=True)
    for flags in (0, NO_CULL):
        g32, g8, _, _ = gpu_ctx.render_points(sc.camera, p, n, seed=rt.SEED, flags=flags)
        assert np.array_equal(bits(g32), bits(f32)) and np.array_equal(g8, u8), flags
    # the oracle's way, as test_gpu_point_table.reference: orc_shade from the point along the oracle's direction, f32 sum in sample order
    lib, osc, pod = orc.load(), orc.OracleScene(flat), sc.camera.to_pod()
    fp = C.POINTER(C.c_float)
    aa = sc.camera.aa_sample_count
    samples = np.zeros((aa, rt.H, rt.W, 3), np.float32)
    for s in range(aa):
        for y, x in zip(*np.nonzero(n[0].any(axis=-1))):
            rc = lib.orc_shade(osc._h, C.byref(pod), C.cast(p[0, y, x].ctypes.data, fp), C.cast(dirs[s, y, x].ctypes.data, fp),
                               rt.SEED, int(y * rt.W + x), s, C.cast(samples[s, y, x].ctypes.data, fp))
            assert rc == 0
    osc.close()
    acc = np.zeros((rt.H, rt.W, 3), np.float32)
    for s in range(aa):
        acc = acc + samples[s]
    r32 = acc / np.float32(aa)
    r8 = np.stack([orc.tonemap_pixel(px, sc.camera.gamma) for px in r32.reshape(-1, 3)]).reshape(rt.H, rt.W, 3)
    assert int((r32.sum(axis=-1) > 0).sum()) >= 100
    rt.assert_within_bars(f32, u8, r32, r8, "point table depth 1")


# ------------------------------------------------------------------------------------------------------------- 6. the counters
def test_counters_on_cfg2(gpu_ctx, orc):
    """The segment count is the oracle's with and without the cull; the class-B paths (a final ray that entered the teapot's root
    box, or hit a sphere) drop, which shows the shortcut fired; the walkers' work list is exactly the class-B paths."""
    sc = scenes.config2(160, 90, 16, 10)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    _, _, _, cnt = orc.OracleScene(flat).render(sc.camera, seed=1, want_u8=False, want_sig=False, want_counters=True)
    f32, _, _, _ = gpu_ctx.render(sc.camera, seed=1, want_u8=False)
    c_cull = gpu_ctx.last_pipeline_counts()
    g32, _, _, _ = gpu_ctx.render(sc.camera, seed=1, want_u8=False, flags=NO_CULL)
    c_plain = gpu_ctx.last_pipeline_counts()
    print(f"cfg2 160x90x16: oracle segments {cnt['segments']}; cull {c_cull}; no cull {c_plain}")
    assert np.array_equal(bits(f32), bits(g32))
    for c in (c_cull, c_plain):
        assert c["segments"] + c["dead_tile_samples"] == cnt["segments"], (c, cnt["segments"])
        assert c["queue_entries"] == c["paths_b"], c
    assert c_cull["paths_b"] < c_plain["paths_b"], (c_cull, c_plain)
