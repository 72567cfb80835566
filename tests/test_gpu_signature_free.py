"""The signature-free render paths (want_sig=False) — the forms bench.py times — against the CPU oracle.

With signatures off, the wavefront pipeline takes the DEAD-TILE shortcut: a 32x32 tile from which the host's f64 frustum
argument (render_plan.cpp tile_masks) proves nothing reachable generates no camera ray, and wf_reduce writes +0.0 for its pixels
without reading a sample slot.  With signatures on the shortcut is off (the signature folds in the RNG state of every
sample), so every parity test that renders with want_sig=True leaves the shortcut, and the SIG = false instantiations of
every kernel, unchecked.  Here each case goes through `check_signature_free`:

  1. want_sig=True  against the oracle: signatures bit-exact, RMS <= 1e-3, max rel err <= 2e-5, u8 <= 1 LSB;
  2. want_sig=False against step 1: f32 and u8 bit for bit (and the sign bits: a dead pixel is +0.0);
  3. want_sig=False against the oracle directly, same f32 / u8 bars;
  4. the pipeline counts: dead_tile_samples > 0 where the scene is built to have dead tiles, == 0 where the design has none
     (a Plane or a ConvexVolume in the list, > 64 list entries, orthographic or defocused cameras), and — over a whole frame —
     segments + dead_tile_samples == the oracle's segment count (a dead sample is one camera ray that hits nothing).

Forms reached (SIG = false side of pt_kernels.hip launch_wf_main / launch_megakernel / launch_megakernel_voted / launch_phong /
launch_branch).  launch_wf_main picks wf_main<SIG=false, V, M, R, I, TOP>: every render runs the camera-ray pass (M=0, I=1) and
later passes without a mesh branch (the lean form, M=0, I=0); a scene with meshes adds M=1 (untextured) or M=2 (maps or a
normal map) for the passes that can meet a mesh hit.

  kind   V R | meshes      M forms     | top tree  TOP | case id of test_wf_main_forms
  plain  0 0 | none        0/I, 0      | off, on   0,1 | plain-none-flat, plain-none-top
  plain  0 0 | untextured  0/I, 0, 1   | off, on   0,1 | plain-mesh-flat, plain-mesh-top
  plain  0 0 | textured    0/I, 0, 2   | off, on   0,1 | plain-tex-flat,  plain-tex-top
  rare   0 1 | none        0/I, 0      | off, on   0,1 | rare-none-flat,  rare-none-top     (a Plane)
  rare   0 1 | untextured  0/I, 0, 1   | off, on   0,1 | rare-mesh-flat,  rare-mesh-top     (a sphere-bounded ConvexVolume)
  rare   0 1 | textured    0/I, 0, 2   | off, on   0,1 | rare-tex-flat,   rare-tex-top      (Plane + sphere volume)
  gv     1 1 | none        0/I, 0      | off, on   0,1 | gv-none-flat,    gv-none-top       (boundary: a Scene of Triangles)
  gv     1 1 | untextured  0/I, 0, 1   | off, on   0,1 | gv-mesh-flat,    gv-mesh-top       (boundary: a cube StaticMesh)
  gv     1 1 | textured    0/I, 0, 2   | off, on   0,1 | gv-tex-flat,     gv-tex-top        (boundary: a cube StaticMesh)

  launch_megakernel        pt_megakernel<L=0, SIG=false>                test_other_kernels[simple-plain-none], [simple-gv-none]
                           pt_megakernel<L=1, SIG=false>                test_other_kernels[simple-plain-mesh], [simple-gv-mesh]
  launch_megakernel_voted  pt_megakernel_voted<L=0, false, 0, V=0>     test_other_kernels[voted-plain-none]
                           pt_megakernel_voted<L=0, false, 0, V=1>     test_other_kernels[voted-gv-none]
                           pt_megakernel_voted<L=1, false, 0, V=0>     test_other_kernels[voted-plain-mesh]
                           pt_megakernel_voted<L=1, false, 0, V=1>     test_other_kernels[voted-gv-mesh]
                           (L: the scene's meshes in LDS, mi_stats.scene_in_lds; a scene without meshes has L = 0)
  launch_branch            pt_branch<false>                     test_other_kernels[recursive-*]
  launch_phong             pt_phong<false>                      test_phong[perspective], test_phong[orthographic]
  launch_walker            (no SIG parameter; reached under the SIG = false wf_main)  test_walker_storage_modes,
                                                                 test_two_stage_meshes
"""
import math

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Camera, ConvexVolume, Dielectric, Isotropic, Lambertian, Metal, MultiContext, Plane, Scene,
                                     Sphere, StaticMesh, Triangle, abi, cgmath, scenes)
from cs397raytracingsp22_amd import Context
from cs397raytracingsp22_amd import dist as pdist
from cs397raytracingsp22_amd.progressive import ProgressiveRender

from test_gpu_edge_cases import _many_triangles
from test_oracle_kat import cube_mesh, cube_triangles

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3


# ------------------------------------------------------------------------------------------------------------------ the check
def _bars(f32, u8, r32, r8, what):
    for ch in range(3):
        rms = float(np.sqrt(np.mean((f32[..., ch].astype(np.float64) - r32[..., ch]) ** 2)))
        assert rms <= RMS_TOL, (what, ch, rms)
    err = np.abs(f32.astype(np.float64) - r32) / np.maximum(1.0, np.abs(r32.astype(np.float64)))
    assert float(err.max()) <= 2e-5, (what, float(err.max()))
    if u8 is not None:
        assert int(np.abs(u8.astype(int) - r8.astype(int)).max()) <= 1, what
    # black is +0.0 on both sides (the dead-tile shortcut writes its pixels without a sample)
    assert np.array_equal(np.signbit(f32), np.signbit(r32)), what


def _win(a, window):
    if window is None:
        return a
    x0, y0, w, h = window
    return a[y0:y0 + h, x0:x0 + w]


def check_signature_free(ctx, orc, sc, seed, window=None, dead=None, upload=True, **render_kw):
    """The four steps of the module docstring.  `dead`: True (the scene is built to have dead tiles), False (the design allows
    none), None (not asserted).  The counts are the wavefront pipeline's: for another variant or Phong shading nothing about
    them is asserted.  Returns the pipeline counts of the signature-free render, and its mi_stats.scene_in_lds."""
    flat = sc.flatten()
    if upload:
        ctx.upload(flat)
    cam = sc.camera
    f32, u8, sig, _ = ctx.render(cam, seed=seed, want_sig=True, **render_kw)
    wavefront = render_kw.get("variant", abi.MI_VARIANT_DEFAULT) in (abi.MI_VARIANT_DEFAULT, abi.MI_VARIANT_WAVEFRONT) and \
        cam.shading_mode == abi.MI_SHADE_PATHTRACE and cam.path_samples == 1
    full = window is None and wavefront
    r32, r8, rsig, cnt = orc.OracleScene(flat).render(cam, seed=seed, window=window, want_counters=full)
    bad = int((_win(sig, window) != rsig).sum())
    assert bad == 0, f"{bad}/{rsig.size} pixels took a different path than the oracle"
    _bars(_win(f32, window), _win(u8, window), r32, r8, "want_sig=True")
    g32, g8, gsig, gst = ctx.render(cam, seed=seed, want_sig=False, **render_kw)
    counts = dict(ctx.last_pipeline_counts(), scene_in_lds=int(gst.scene_in_lds))
    assert gsig is None
    assert np.array_equal(g32, f32) and np.array_equal(g8, u8), "want_sig=False differs from want_sig=True"
    assert np.array_equal(np.signbit(g32), np.signbit(f32))
    _bars(_win(g32, window), _win(g8, window), r32, r8, "want_sig=False")
    if not wavefront:
        assert dead is None
    elif dead is True:
        assert counts["dead_tile_samples"] > 0, counts
    elif dead is False:
        assert counts["dead_tile_samples"] == 0, counts
    if full:
        assert counts["segments"] + counts["dead_tile_samples"] == cnt["segments"], (counts, cnt["segments"])
    return counts


def _fraction(counts, cam):
    return counts["dead_tile_samples"] / float(cam.screen_width * cam.screen_height * cam.aa_sample_count)


# ------------------------------------------------------------------------------------------------------------ the forms
GREY = Lambertian(albedo=(0.6, 0.6, 0.6))
LIGHT = Lambertian(albedo=(0.7, 0.7, 0.7), emission=(2.0, 2.0, 2.0))


def _cam(w=128, h=96, spp=8, depth=6, **kw):
    args = dict(eyepoint=(0.0, 1.0, 5.0), view_dir=(0.0, -0.05, -1.0), up=(0.0, 1.0, 0.0), path_depth=depth, path_samples=1,
                screen_width=w, screen_height=h, focal_length=0.6, focus_dist=5.0, lens_radius=0.0, aa_sample_count=spp,
                max_trace_dist=100.0, gamma=2.0)
    args.update(kw)
    return Camera(**args)


def _textures():
    t = scenes.load_asset_textures()
    return [t["green"], None, None, None, t["normal_test_png"]]


def form_scene(kind, meshes, top, **cam_kw):
    """A small cluster around (0, 1, 0) seen from z = 5: the frame's outer tiles see nothing (dead when nothing is unmasked)."""
    rng = np.random.default_rng({"plain": 1, "rare": 2, "gv": 3}[kind] * 10 + {"none": 0, "mesh": 1, "tex": 2}[meshes])
    objs = [Sphere((-0.6, 1.0, 0.0), 0.45, Metal(albedo=(0.8, 0.7, 0.6), emission=(0.3, 0.2, 0.1), roughness=0.2)),
            Sphere((0.7, 0.8, 0.3), 0.35, Dielectric(1.5)),
            Sphere((0.0, 2.1, -0.4), 0.3, LIGHT),
            Triangle((-0.8, 0.1, -0.8), (0.8, 0.1, -0.8), (0.0, 0.9, -1.4), Lambertian(albedo=(0.5, 0.6, 0.4), emission=(0.1, 0.3, 0.2))),
            Triangle((-0.4, 1.9, -1.0), (0.5, 1.9, -1.0), (0.0, 2.5, -1.0), LIGHT)]
    if top:                                     # >= 96 list Triangles: the scene compiler builds a top-level tree over them
        objs += _many_triangles(rng, 100, lo=(-1.3, 0.0, -1.3), hi=(1.3, 2.4, 1.0), size=0.12)
    if meshes == "mesh":
        objs.append(StaticMesh(scenes.load_asset_mesh("teapot"), Lambertian(albedo=(0.6, 0.3, 0.2), emission=(0.2, 0.2, 0.2)),
                               [None] * 5, cgmath.mul(cgmath.from_translation((0.2, 0.6, 0.6)), cgmath.from_scale(0.25))))
    elif meshes == "tex":
        objs.append(StaticMesh(scenes.load_asset_mesh("cube"), None, _textures(),
                               cgmath.mul(cgmath.from_translation((0.3, 0.7, 0.5)), cgmath.from_angle_y(35.0), cgmath.from_scale(0.3))))
    if kind == "rare":
        if meshes != "mesh":
            objs.append(Plane((0.0, -0.2, 0.0), (0.0, 1.0, 0.0), Lambertian(albedo=(0.4, 0.4, 0.4), emission=(0.05, 0.05, 0.05))))
        if meshes != "none":
            objs.append(ConvexVolume(Sphere((-0.9, 1.6, 0.2), 0.4, GREY), Isotropic(albedo=(0.9, 0.8, 0.7)), 2.0))
    elif kind == "gv":
        if meshes == "none":
            inner = Scene(Camera(), cube_triangles(0.4, 1.0))
            objs.append(ConvexVolume(inner, Isotropic(albedo=(0.5, 0.8, 0.9)), 2.5))
        else:
            cube = StaticMesh(cube_mesh(-0.3, 0.3), GREY, [None] * 5, cgmath.from_translation((-0.9, 1.6, 0.2)))
            objs.append(ConvexVolume(cube, Isotropic(albedo=(0.9, 0.7, 0.5)), 1.5))
    objs = [objs[i] for i in rng.permutation(len(objs))]
    return Scene(_cam(**cam_kw), objs)


FORMS = [(k, m, t) for k in ("plain", "rare", "gv") for m in ("none", "mesh", "tex") for t in (False, True)]


def builds_top_tree(sc):
    """The scene compiler's rule (mi_rt.cpp, kTopMinTris): the list's Triangles get a top-level tree when >= 96 of them have
    |e1| |e2| <= 32 x the median product.  The library exposes no flag for it, so the TOP = 1 cases check the rule here."""
    prod = []
    for o in sc.objects:
        if isinstance(o, Triangle):
            a, b, c = (np.float32(v) for v in (o.a, o.b, o.c))
            prod.append(np.linalg.norm((b - a).astype(np.float64)) * np.linalg.norm((c - a).astype(np.float64)))
    if len(prod) < 96:
        return False
    prod = np.asarray(prod)
    big = 32.0 * np.partition(prod, len(prod) // 2)[len(prod) // 2]
    return int((np.isfinite(prod) & (prod <= big)).sum()) >= 96


@pytest.mark.parametrize("kind,meshes,top", FORMS, ids=[f"{k}-{m}-{'top' if t else 'flat'}" for k, m, t in FORMS])
def test_wf_main_forms(gpu_ctx, orc, kind, meshes, top):
    sc = form_scene(kind, meshes, top)
    flat = sc.flatten()
    assert (flat.desc.n_meshes > 0) == (meshes != "none")
    assert builds_top_tree(sc) == top
    # dead tiles need every entry maskable: no Plane / ConvexVolume, at most 64 list entries (the tree's 100 are too many)
    check_signature_free(gpu_ctx, orc, sc, seed=3, dead=(kind == "plain" and not top))


OTHER = [(v, k, m) for v in ("simple", "voted", "recursive") for k in ("plain", "gv") for m in ("none", "mesh")]


@pytest.mark.parametrize("variant,kind,meshes", OTHER, ids=[f"{v}-{k}-{m}" for v, k, m in OTHER])
def test_other_kernels(gpu_ctx, orc, variant, kind, meshes):
    """pt_megakernel / pt_megakernel_voted (with and without the general-volume branch, scene in LDS or not) / pt_branch with
    SIG = false.  gv-none: the medium's boundary is a Scene of Triangles, so the gv branch runs without a mesh."""
    v = {"simple": abi.MI_VARIANT_SIMPLE, "voted": abi.MI_VARIANT_VOTED, "recursive": abi.MI_VARIANT_RECURSIVE}[variant]
    sc = form_scene(kind, meshes, False, w=96, h=64)
    counts = check_signature_free(gpu_ctx, orc, sc, seed=5, variant=v)
    if variant != "recursive":
        assert counts["scene_in_lds"] == (meshes == "mesh")             # the L of the table above


@pytest.mark.parametrize("projection", ["perspective", "orthographic"])
def test_phong(gpu_ctx, orc, projection):
    sc = form_scene("plain", "tex", False, w=96, h=64, shading_mode=abi.MI_SHADE_PHONG,
                    projection_mode=abi.MI_PROJ_PERSPECTIVE if projection == "perspective" else abi.MI_PROJ_ORTHOGRAPHIC)
    sc.point_light_pos = (0.5, 4.0, 2.5)
    sc.ambient = (0.05, 0.1, 0.15)
    check_signature_free(gpu_ctx, orc, sc, seed=6)


@pytest.mark.parametrize("camera", ["orthographic", "defocus"])
def test_no_dead_tiles_without_a_pinhole(gpu_ctx, orc, camera):
    """The frustum argument needs every ray to leave the eye: an orthographic or a defocused camera keeps every tile alive."""
    kw = {"orthographic": dict(projection_mode=abi.MI_PROJ_ORTHOGRAPHIC, eyepoint=(0.0, 1.0, 5.0)),
          "defocus": dict(lens_radius=0.05)}[camera]
    sc = form_scene("plain", "mesh", False, **kw)
    check_signature_free(gpu_ctx, orc, sc, seed=7, dead=False)


def test_walker_storage_modes(orc):
    """Every storage mode of the reference-tree walker (MI_RT_WF_TRAV_LDS) under the SIG = false wf_main, dead tiles live."""
    from test_gpu_walkers import render_with_env
    sc = form_scene("plain", "mesh", False)
    flat = sc.flatten()
    r32, r8, _, _ = orc.OracleScene(flat).render(sc.camera, seed=4)
    for mode in (0, 4, 5, 6):
        env = {"MI_RT_WF_TRAV_LDS": mode}
        f32, sig = render_with_env(env, flat, sc.camera, 4, flags=abi.MI_OPT_REFERENCE_WALK)
        g32, gsig = render_with_env(env, flat, sc.camera, 4, flags=abi.MI_OPT_REFERENCE_WALK, want_sig=False)
        assert gsig is None and np.array_equal(g32, f32), mode
        _bars(g32, None, r32, None, f"mode {mode}")


@pytest.mark.parametrize("name", ["teapot", "head"])
def test_two_stage_meshes(gpu_ctx, orc, name):
    """The two-stage (candidate list, then exact replay) mesh walk: forced on the teapot, the HEAD scene's default."""
    if name == "teapot":
        sc = scenes.config2(128, 96, 8, 8)
        sc.objects = [o for o in sc.objects if not isinstance(o, Plane)]
        kw = dict(flags=abi.MI_OPT_TWO_STAGE)
    else:
        sc = scenes.head_scene(96, 80, 8, 10)
        kw = {}
    check_signature_free(gpu_ctx, orc, sc, seed=12, dead=None if name == "teapot" else False, **kw)


# -------------------------------------------------------------------------------------------- attacks on the dead-tile proof
def _basis(cam):
    """tile_masks' f64 camera basis: R = [normalize(view x up), up, -view] (tracing.rs:185-189, not orthogonalised)."""
    view = np.asarray(np.float32(cam.view_dir), np.float64)
    up = np.asarray(np.float32(cam.up), np.float64)
    c0 = np.cross(view, up)
    return np.column_stack([c0 / np.linalg.norm(c0), up, -view])


def pixel_point(cam, px, py, t):
    """The world point at parameter t along the ray through image position (px, py) (pixel centres at integers), as tile_masks'
    dir(): eye + t * R (p (px - W/2 + 1/2), p (1/2 + H/2 - py), -focal)."""
    W, H = cam.screen_width, cam.screen_height
    p = 1.0 / H
    q = np.array([p * (px - 0.5 * W + 0.5), p * (0.5 + 0.5 * H - py), -float(np.float32(cam.focal_length))])
    return np.asarray(np.float32(cam.eyepoint), np.float64) + t * (_basis(cam) @ q)


def project(cam, X):
    """Inverse of pixel_point: image positions (px, py) of world points X [..., 3] (in front of the eye)."""
    W, H = cam.screen_width, cam.screen_height
    p = 1.0 / H
    q = np.linalg.solve(_basis(cam), (np.asarray(X, np.float64) - np.asarray(np.float32(cam.eyepoint), np.float64)).reshape(-1, 3).T).T
    s = -float(np.float32(cam.focal_length)) / q[:, 2]
    assert (s > 0).all()
    return q[:, 0] * s / p + 0.5 * W - 0.5, 0.5 + 0.5 * H - q[:, 1] * s / p


def _fib_sphere(n=20000):
    k = np.arange(n) + 0.5
    z = 1.0 - 2.0 * k / n
    a = math.pi * (1.0 + 5 ** 0.5) * k
    r = np.sqrt(1.0 - z * z)
    return np.stack([r * np.cos(a), r * np.sin(a), z], axis=1)


def place(cam, outline, px, py, t, edge, target):
    """Move a rigid point set (`outline(centre)` -> its silhouette points) to image position (px, py) at ray parameter t, then
    along the image x axis until its extreme x (`edge` = 'min' or 'max') is `target` (f64, to 1e-3 px).  Returns the centre."""
    for _ in range(12):
        c = pixel_point(cam, px, py, t)
        xs, _ = project(cam, outline(c))
        ext = xs.min() if edge == "min" else xs.max()
        if abs(ext - target) < 1e-4:
            break
        px += target - ext
    assert abs(ext - target) < 1e-3, (ext, target)
    return c


EDGE_OFFSETS = (0.25, 0.75, 1.25, 1.75)


def tile_edge_scene(spp, side, kind0):
    """9 x 3 tiles (288 x 96).  Rows 0 and 2: columns 0, 2, 4, 6, 8 hold nothing (dead unless the proof keeps them); in each of
    the columns 1, 3, 5, 7 sits one tiny emitter whose silhouette lies EDGE_OFFSETS[k] px outside the pixel-centre footprint of
    the dead neighbour — to its right (side '+': reached only by positive jitter) or to its left (side '-').  Row 0 holds
    spheres (kind0 'sphere') or cube meshes whose world box corner is the extreme (kind0 'mesh'), row 2 list Triangles.
    Row 1: a non-emitting backdrop of small list Triangles, >= 8 px away from rows 0 and 2, keeps its tiles live.  Skewed,
    non-unit view_dir / up, lens_radius 0."""
    cam = Camera(eyepoint=(0.3, -0.2, 1.0), view_dir=(0.1, -0.08, -1.15), up=(0.07, 0.93, 0.05), path_depth=4, path_samples=1,
                 screen_width=288, screen_height=96, focal_length=0.7, focus_dist=4.0, lens_radius=0.0, aa_sample_count=spp,
                 max_trace_dist=100.0, gamma=2.0)
    T = 6.0                                                              # ray parameter of every object
    emit = Lambertian(albedo=(0.5, 0.5, 0.5), emission=(4.0, 3.0, 2.0))
    dark = Lambertian(albedo=(0.6, 0.6, 0.6))
    objs = []
    rng = np.random.default_rng(spp * 7 + (side == "+"))
    for j in range(24):                                                  # backdrop: row 1, y in [40, 56]
        cx, cy = 8.0 + 272.0 * j / 23.0, rng.uniform(44.0, 52.0)
        pts = [pixel_point(cam, cx + dx, cy + dy, T) for dx, dy in ((-6, -4), (6, -4), (0, 4))]
        objs.append(Triangle(*[tuple(map(float, q)) for q in pts], dark))
    sph = _fib_sphere()
    for row in (0, 2):
        for k, d in enumerate(EDGE_OFFSETS):
            col = 2 * k + 1                                              # the emitter's tile column; the dead ones are col +- 1
            if side == "+":                                              # right of the dead column col - 1
                target, edge, px = 32.0 * col - 1.0 + d, "min", 32.0 * col + 6.0
            else:                                                        # left of the dead column col + 1
                target, edge, px = 32.0 * (col + 1) - d, "max", 32.0 * (col + 1) - 7.0
            py = 16.0 + 64.0 * (row == 2) + (-3.0 if k % 2 else 3.0)
            if row == 2:                                                 # a triangle: vertices at parameter T, exact silhouette
                xs = np.array([0.0, 9.0, 4.0]) + rng.uniform(-0.5, 0.5, 3)
                ys = np.array([-4.0, -3.0, 5.0])
                xs += (target - xs.min()) if edge == "min" else (target - xs.max())
                pts = [pixel_point(cam, x, py + y, T) for x, y in zip(xs, ys)]
                objs.append(Triangle(*[tuple(map(float, q)) for q in pts], emit))
            elif kind0 == "sphere":
                r = float(np.linalg.norm(pixel_point(cam, 0.0, 0.0, T) - pixel_point(cam, 4.0, 0.0, T)))
                c = place(cam, lambda c: c + r * sph, px, py, T, edge, target)
                objs.append(Sphere(tuple(map(float, c)), r, emit))
            else:                                                        # axis-aligned cube: its box corners are its vertices
                h = 0.5 * float(np.linalg.norm(pixel_point(cam, 0.0, 0.0, T) - pixel_point(cam, 6.0, 0.0, T)))
                corners = np.array([(x, y, z) for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64)
                c = place(cam, lambda c: c + corners, px, py, T, edge, target)
                c32 = np.float32(c)                                      # the translation the library sees
                xs, _ = project(cam, c32.astype(np.float64) + corners)
                assert abs((xs.min() if edge == "min" else xs.max()) - target) < 1e-2
                objs.append(StaticMesh(cube_mesh(-h, h), emit, [None] * 5, cgmath.from_translation(tuple(map(float, c32)))))
    return Scene(cam, objs)


TILE_EDGE = [(spp, side, kind0) for spp in (1, 2, 3, 8, 24) for side in ("+", "-") for kind0 in ("sphere", "mesh")]


@pytest.mark.parametrize("spp,side,kind0", TILE_EDGE, ids=[f"spp{s}{d}-{k}" for s, d, k in TILE_EDGE])
def test_objects_just_outside_a_dead_tile(gpu_ctx, orc, spp, side, kind0):
    """The x jitter of a sample reaches from -1 px to +0.21 / +0.82 / +0.94 / +0.98 px (n = 2 / 3 / 8 / 24) past its pixel centre
    (tracing.rs:166-173; n = 1: exactly -1 px).  So an emitter 0.25 or 0.75 px outside a dead tile's footprint is hit by some of
    that tile's rays on side '-' at every n, and on side '+' only for n >= 3 (0.75: n = 3 reaches it through +0.82 px); one 1.25 or
    1.75 px out is hit by none.  Either way the tile's image must equal the oracle's, signature-free included."""
    sc = tile_edge_scene(spp, side, kind0)
    counts = check_signature_free(gpu_ctx, orc, sc, seed=31, dead=True)
    print(f"tile edge spp {spp} side {side} {kind0}: dead fraction {_fraction(counts, sc.camera):.3f}")


def beyond_one_pixel_scene(offset=1.035):
    """3 x 8 tiles (96 x 256), n = 31 samples: the x jitter of sample i = 30 reaches +1.045 px (floor(30 / 5) / sqrt(31) + (30 - 15.5)
    / 31 - 1/2), past the +-1 px a footprint widened by one pixel would cover.  In column 1, Triangles' left edges lie `offset` px
    right of column 0's last pixel centre (the 1.01 scaling of the mask test moves them 0.028 px closer: still culled by a 1 px
    margin); column 0 sees it only through those samples (rand_x = 30, one
    pixel in 31), column 2 sees nothing.  The Triangles are fat enough for the conditioning guard, so they are maskable."""
    cam = Camera(eyepoint=(0.3, -0.2, 1.0), view_dir=(0.1, -0.08, -1.15), up=(0.07, 0.93, 0.05), path_depth=3, path_samples=1,
                 screen_width=96, screen_height=256, focal_length=0.7, focus_dist=4.0, lens_radius=0.0, aa_sample_count=31,
                 max_trace_dist=100.0, gamma=2.0)
    emit = Lambertian(albedo=(0.5, 0.5, 0.5), emission=(4.0, 3.0, 2.0))
    x = 31.0 + offset
    objs = []
    for j in range(16):                                                  # two per tile row: short edges keep them well conditioned
        y0 = 16.0 * j
        pts = [pixel_point(cam, px, py, 6.0) for px, py in ((x, y0 + 0.5), (x, y0 + 15.5), (x + 8.5, y0 + 8.0))]
        objs.append(Triangle(*[tuple(map(float, q)) for q in pts], emit))
    return Scene(cam, objs)


def test_jitter_past_one_pixel(gpu_ctx, orc):
    """Non-square n reaches further than +1 px (render_plan.cpp tile_masks); the 2 px margin must keep column 0 alive."""
    sc = beyond_one_pixel_scene()
    counts = check_signature_free(gpu_ctx, orc, sc, seed=41, dead=True)
    r32, _, _, _ = orc.OracleScene(sc.flatten()).render(sc.camera, seed=41, want_u8=False, want_sig=False)
    assert r32[:, :32].max() > 0.0 and not r32[:, 64:].any()           # the scene does what it is built for
    print(f"jitter past one pixel: dead fraction {_fraction(counts, sc.camera):.3f}")


def clustered_scene(seed):
    """A random skewed, non-unit camera basis (as tests/test_gpu_tile_masks.py scatter_scene) and small, well-conditioned Triangles
    and Spheres placed through it in the left half of the frame at random depths: the tiles of the right half are dead, the
    others hold objects at random positions relative to the tile edges."""
    rng = np.random.default_rng(700 + seed)
    view = rng.normal(size=3); view /= np.linalg.norm(view); view *= rng.uniform(0.7, 1.4)
    up = rng.normal(size=3); up /= np.linalg.norm(up); up *= rng.uniform(0.8, 1.3)
    if abs(np.dot(view, up)) > 0.8 * np.linalg.norm(view) * np.linalg.norm(up):
        up = np.cross(view, up) + 0.3 * up
    cam = Camera(eyepoint=tuple(map(float, rng.uniform(-1, 1, 3))), view_dir=tuple(map(float, view)), up=tuple(map(float, up)),
                 path_depth=4, path_samples=1, screen_width=int(rng.integers(160, 260)), screen_height=int(rng.integers(70, 150)),
                 focal_length=float(rng.uniform(0.4, 1.0)), focus_dist=5.0, lens_radius=0.0, aa_sample_count=int(rng.choice([1, 3, 4, 8, 9])),
                 max_trace_dist=25.0, gamma=2.0)                       # short enough for every Triangle to pass the guard
    mats = [Lambertian(albedo=(0.7, 0.7, 0.7), emission=(1.5, 1.2, 0.9)), Metal(albedo=(0.8, 0.6, 0.4), roughness=0.2),
            Dielectric(idx_of_refraction=1.5), Lambertian(albedo=(0.2, 0.6, 0.3))]
    W, H = cam.screen_width, cam.screen_height
    objs = []
    for k in range(20):
        px, py, t, R = rng.uniform(0.05 * W, 0.5 * W), rng.uniform(0.05 * H, 0.95 * H), rng.uniform(2.0, 8.0), rng.uniform(4.0, 9.0)
        mat = mats[int(rng.integers(len(mats)))]
        if k % 3:
            a0 = rng.uniform(0, 2 * np.pi)
            pts = [pixel_point(cam, px + R * np.cos(a0 + 2.1 * q), py + R * np.sin(a0 + 2.1 * q), t * rng.uniform(0.98, 1.02))
                   for q in range(3)]
            objs.append(Triangle(*[tuple(map(float, v)) for v in pts], mat))
        else:
            r = R * float(np.linalg.norm(pixel_point(cam, px, py, t) - pixel_point(cam, px + 1.0, py, t)))
            objs.append(Sphere(tuple(map(float, pixel_point(cam, px, py, t))), r, mat))
    return Scene(cam, objs)


@pytest.mark.parametrize("seed", list(range(16)))
def test_random_skewed_cameras_with_dead_tiles(gpu_ctx, orc, seed):
    sc = clustered_scene(seed)
    counts = check_signature_free(gpu_ctx, orc, sc, seed=seed, dead=True)
    print(f"clustered seed {seed}: dead fraction {_fraction(counts, sc.camera):.3f}")


def _eye_case(case):
    eye = np.array([0.2, 1.0, 3.0])
    light = Lambertian(albedo=(0.6, 0.6, 0.6), emission=(1.5, 1.5, 1.5))
    cam = _cam(w=128, h=96, spp=9, depth=5, eyepoint=tuple(eye), view_dir=(0.05, 0.0, -0.9), up=(0.0, 1.1, 0.1))
    objs = [Sphere((0.0, 1.0, -2.0), 0.5, light), Sphere((0.5, 0.7, -2.6), 0.3, Metal(albedo=(0.8, 0.8, 0.8), roughness=0.1))]
    front_tri = Triangle((-0.6, 0.4, -2.5), (0.5, 0.5, -2.5), (0.0, 1.6, -2.6), GREY)
    if case == "behind":                                                 # small objects in the cone behind the eye
        objs += [front_tri, Sphere(tuple(eye + (0.1, 0.1, 1.5)), 0.3, light), Sphere(tuple(eye + (-0.5, 0.2, 4.0)), 0.8, light),
                 Triangle(tuple(eye + (-0.3, -0.3, 1.2)), tuple(eye + (0.3, -0.3, 1.2)), tuple(eye + (0.0, 0.3, 1.3)), light)]
    elif case == "straddle":                                             # across the eye's plane, off to the left
        objs += [front_tri, Sphere(tuple(eye + (-2.5, 0.0, 0.0)), 1.0, light),
                 Triangle(tuple(eye + (-4.0, -0.5, -1.5)), tuple(eye + (-2.6, 0.0, 1.5)), tuple(eye + (-3.5, 1.0, 0.2)), light)]
    elif case == "in_plane":                                             # the eye lies in the triangle's plane y = 1
        objs += [front_tri, Triangle((-4.0, 1.0, -1.0), (-1.0, 1.0, -1.0), (-2.0, 1.0, 6.0), light)]
    elif case == "far":                                                  # max_trace_dist 1e30 (spheres only: a Triangle's guard
        cam.max_trace_dist = 1e30                                        # G grows with it and keeps the Triangle everywhere)
        objs += [Sphere((40.0, 30.0, -200.0), 10.0, light)]
    return Scene(cam, objs)


@pytest.mark.parametrize("case", ["behind", "straddle", "in_plane", "far"])
def test_geometry_around_the_eye(gpu_ctx, orc, case):
    sc = _eye_case(case)
    # a triangle the eye lies in cannot be masked (guard G): it stays in every tile, so no tile is dead
    check_signature_free(gpu_ctx, orc, sc, seed=17, dead=(case != "in_plane"))


RAGGED = [(w, h) for w in (1, 31, 33, 65, 203) for h in (1, 33, 117)]


@pytest.mark.parametrize("w,h", RAGGED, ids=[f"{w}x{h}" for w, h in RAGGED])
def test_ragged_frames(gpu_ctx, orc, w, h):
    sc = form_scene("plain", "mesh", False, w=w, h=h, spp=4, depth=5)
    counts = check_signature_free(gpu_ctx, orc, sc, seed=19)
    if w >= 65 and h >= 33:                                               # tile columns the centred cluster does not reach
        assert counts["dead_tile_samples"] > 0


# ------------------------------------------------------------------------------------------- batching, ranges, ranks, reuse
def test_several_batches(gpu_ctx, orc):
    sc = form_scene("plain", "mesh", False, spp=25)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    ref32, ref8, _, _ = gpu_ctx.render(sc.camera, seed=11, want_sig=True)
    npix = pdist.tiles_padded(sc.camera.screen_width, sc.camera.screen_height, 1) * pdist.TILE_PIXELS
    bytes_per_path = 2 * 6 * 16 + 16
    small = Context(0)
    try:
        small.upload(flat)
        f32, u8, _, _ = small.render(sc.camera, seed=11, max_state_bytes=npix * 7 * bytes_per_path)          # 7 + 7 + 7 + 4
        c = small.last_pipeline_counts()
        batched_launches = small.last_pipeline_ms()["launches"]
    finally:
        small.close()
    gpu_ctx.render(sc.camera, seed=11)
    assert batched_launches > gpu_ctx.last_pipeline_ms()["launches"]
    assert np.array_equal(f32, ref32) and np.array_equal(u8, ref8)
    assert c["dead_tile_samples"] > 0
    r32, r8, _, cnt = orc.OracleScene(flat).render(sc.camera, seed=11, want_counters=True)
    assert c["segments"] + c["dead_tile_samples"] == cnt["segments"]
    _bars(f32, u8, r32, r8, "batched")


def test_progressive_slices_without_signatures(gpu_ctx, tmp_path):
    sc = form_scene("plain", "tex", False, spp=16)
    gpu_ctx.upload(sc.flatten())
    want, _, _, _ = gpu_ctx.render(sc.camera, seed=9, want_u8=False, want_sig=True)
    plain, _, _, _ = gpu_ctx.render(sc.camera, seed=9, want_u8=False)
    assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] > 0
    pr = ProgressiveRender(gpu_ctx, sc.camera, seed=9, want_sig=False)
    assert pr.advance(3).samples == 3 * sc.camera.screen_width * sc.camera.screen_height
    assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] > 0
    pr.advance(6)
    ckpt = str(tmp_path / "part.npz")
    pr.save(ckpt)
    ctx2 = Context(0)
    try:
        ctx2.upload(sc.flatten())
        pr2 = ProgressiveRender.resume(ctx2, sc.camera, ckpt, want_sig=False)
        pr2.advance(10 ** 6)
        got, got_sig = pr2.result()
    finally:
        ctx2.close()
    assert got_sig is None
    assert np.array_equal(got, plain) and np.array_equal(got, want)


LOOPBACK = {
    "cfg2": lambda: scenes.config2(203, 117, 16, 10),                   # 7 x 4 tiles, ragged edges; columns 0 and 6 dead
    "cfg2_1080p": lambda: scenes.config2(1920, 1080, 4, 10),           # the benchmarked frame: dead columns left and right
    "even": lambda: form_scene("plain", "mesh", False, w=192, h=96, spp=8),   # 6 tile columns: worlds 2, 3, 8 pad the stride
}


@pytest.mark.parametrize("scene", sorted(LOOPBACK))
@pytest.mark.parametrize("n", [2, 3, 8])
def test_loopback_ranks_without_signatures(n, scene):
    """mi_multi_render's N >= 2 code without signatures: rank r owns tiles slot * world + r of the coprime grid, so wf_main and
    wf_reduce must look up the dead bit of THAT tile.  Bit-identical to one context's signature render."""
    sc = LOOPBACK[scene]()
    flat = sc.flatten()
    one = Context(0)
    try:
        one.upload(flat)
        ref32, ref8, _, _ = one.render(sc.camera, seed=3, want_sig=True)
        one.render(sc.camera, seed=3)
        single = one.last_pipeline_counts()["dead_tile_samples"]
    finally:
        one.close()
    assert single > 0
    m = MultiContext.loopback(n)
    try:
        m.upload(flat)
        f32, u8, sig, _ = m.render(sc.camera, seed=3, want_sig=False)
        dead = sum(m.context(r).last_pipeline_counts()["dead_tile_samples"] for r in range(n))
    finally:
        m.close()
    assert sig is None
    assert np.array_equal(f32, ref32) and np.array_equal(u8, ref8)
    assert np.array_equal(np.signbit(f32), np.signbit(ref32))
    assert dead == single                                                 # the surplus columns hold no pixel: not counted
    print(f"loopback {scene} n={n}: dead fraction {_fraction({'dead_tile_samples': dead}, sc.camera):.3f}")


def test_stale_state_across_uploads(orc):
    """One context, one camera: a fully lit scene, then a scene with dead tiles, then one with an emitter in a formerly dead
    tile (the tile-mask cache is keyed on the camera: upload must invalidate it), then the same plus a Plane (no dead tile)."""
    lit = form_scene("rare", "none", False)                              # a Plane: every tile alive
    cam = lit.camera
    base = form_scene("plain", "mesh", False)
    base.camera = cam
    corner = pixel_point(cam, 12.0, 10.0, 6.0)                           # inside tile (0, 0), dead in `base`
    moved = Scene(cam, base.objects + [Sphere(tuple(map(float, corner)), 0.3, LIGHT)])
    planed = Scene(cam, moved.objects + [Plane((0.0, -0.3, 0.0), (0.0, 1.0, 0.0), GREY)])
    ctx = Context(0)
    try:
        ctx.upload(lit.flatten())
        ctx.render(cam, seed=2)
        assert ctx.last_pipeline_counts()["dead_tile_samples"] == 0
        c1 = check_signature_free(ctx, orc, base, seed=2, dead=True)
        g32, _, _, _ = ctx.render(cam, seed=2)
        assert not g32[:32, :32].any() and not np.signbit(g32[:32, :32]).any()        # tile (0, 0) is dead: exactly +0.0
        c2 = check_signature_free(ctx, orc, moved, seed=2, dead=True)
        g32, _, _, _ = ctx.render(cam, seed=2)
        assert g32[:32, :32].max() > 0.0                                 # the emitter in tile (0, 0) is seen
        assert c2["dead_tile_samples"] < c1["dead_tile_samples"]
        check_signature_free(ctx, orc, planed, seed=2, dead=False)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------ the benchmarked frames at stated sizes
def test_cfg2_1080p_256spp_golden(gpu_ctx):
    """The exact frame bench.py times (want_sig=False), against the committed golden window — no oracle in the loop."""
    from test_golden import CASES, load
    f32, u8, _, (x0, y0, w, h), seed = load("cfg2_1080p_256spp")
    sc = CASES["cfg2_1080p_256spp"]()
    gpu_ctx.upload(sc.flatten())
    g32, g8, _, _ = gpu_ctx.render(sc.camera, seed=seed)
    assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] > 0
    _bars(g32[y0:y0 + h, x0:x0 + w], g8[y0:y0 + h, x0:x0 + w], f32, u8, "cfg2 1080p")


@pytest.mark.parametrize("name", ["cfg4_drone_480x270_16spp", "cfg5_subsurface_480x270_64spp_d50", "head_200x200_16spp"])
def test_goldens_without_signatures(gpu_ctx, name):
    from test_golden import CASES, load
    f32, u8, _, (x0, y0, w, h), seed = load(name)
    sc = CASES[name]()
    gpu_ctx.upload(sc.flatten())
    g32, g8, _, _ = gpu_ctx.render(sc.camera, seed=seed)
    _bars(g32[y0:y0 + h, x0:x0 + w], g8[y0:y0 + h, x0:x0 + w], f32, u8, name)


@pytest.mark.parametrize("name", ["config4", "config5"])
def test_full_size_frames_equal_their_signature_renders(gpu_ctx, name):
    """cfg4 (1080p, 256 spp, 2048^2 maps) and cfg5 (1080p, 4096 spp, depth 50) as BASELINE states them: the timed form equals the
    signature render bit for bit (which test_gpu_tiles pins against the oracle)."""
    sc = scenes.config4() if name == "config4" else scenes.config5()
    gpu_ctx.upload(sc.flatten())
    f32, u8, _, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    g32, g8, _, _ = gpu_ctx.render(sc.camera, seed=1)
    assert np.array_equal(g32, f32) and np.array_equal(g8, u8)
    assert np.array_equal(np.signbit(g32), np.signbit(f32))
