"""The render planner, host side (CPU only): cs397raytracingsp22_amd/csrc/render_plan.cpp — the tile grid, the primary-ray tile
masks (tile_masks) with the dead-sample count taken from them, and the wavefront pipeline's batch arithmetic — run through
tests/cpp/render_plan_shim.cpp on scenes compiled by the product's own scene compiler, no GPU and no libmi_rt.so.

The mask words and dead-sample counts of tests/golden/render_plan_masks.json were recorded from the tile_masks that lived in
mi_rt.cpp before the planner was split out; the planner must reproduce them bit for bit."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from cs397raytracingsp22_amd import Camera, ConvexVolume, Isotropic, Lambertian, Plane, Scene, Sphere, Triangle, abi, dist, scenes
from test_gpu_signature_free import beyond_one_pixel_scene, tile_edge_scene
from test_gpu_tile_masks import mesh_scene, scatter_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs397raytracingsp22_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "render_plan_masks.json")
WORLDS = (1, 3, 8)
DEAD = 1 << 63


class PlanQuery(C.Structure):          # tests/cpp/render_plan_shim.cpp
    _fields_ = [("scene", C.POINTER(abi.mi_scene_desc)), ("cam", C.POINTER(abi.mi_camera_desc)), ("flags", C.c_uint32),
                ("world", C.c_int32), ("words", C.POINTER(C.c_uint64)), ("words_cap", C.c_uint64),
                ("npix", C.c_uint32), ("spp", C.c_uint32), ("max_state_bytes", C.c_uint64), ("free_bytes", C.c_uint64),
                ("two_stage", C.c_int32), ("applies", C.c_int32), ("n_words", C.c_uint64), ("dead_samples", C.c_uint64 * 8),
                ("pixels", C.c_uint64 * 8), ("s_batch", C.c_uint32), ("region", C.c_uint32), ("cap", C.c_uint32),
                ("state_bytes", C.c_uint64), ("samp_bytes", C.c_uint64), ("acc_bytes", C.c_uint64), ("err", C.c_char * 512)]


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    so = tmp_path_factory.mktemp("rp") / "render_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-shared",
                    os.path.join(CSRC, "render_plan.cpp"), os.path.join(CSRC, "scene_compile.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "render_plan_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.render_plan_query.argtypes = [C.c_int, C.POINTER(PlanQuery)]
    lib.render_plan_query.restype = C.c_int
    return lib


def masks(lib, flat, cam, world, flags=0):
    """(rc, applies, mask words, per-rank dead samples, per-rank pixels) of the scene `flat` under the Camera `cam`."""
    pod = cam.to_pod()
    cap = 2 * 1100 * 40
    words = (C.c_uint64 * cap)()
    q = PlanQuery(scene=C.pointer(flat.desc), cam=C.pointer(pod), flags=flags, world=world, words=words, words_cap=cap)
    rc = lib.render_plan_query(0, C.byref(q))
    assert rc > -100, rc
    w = np.frombuffer(words, np.uint64, count=q.n_words).copy()
    return rc, bool(q.applies), w, [int(q.dead_samples[r]) for r in range(world)], [int(q.pixels[r]) for r in range(world)]


def batch(lib, npix, spp, max_state_bytes=0, free_bytes=0, two_stage=False):
    q = PlanQuery(npix=npix, spp=spp, max_state_bytes=max_state_bytes, free_bytes=free_bytes, two_stage=int(two_stage))
    rc = lib.render_plan_query(1, C.byref(q))
    return rc, q


def digest(words):
    return hashlib.sha256(words.astype("<u8").tobytes()).hexdigest()


# ---------------------------------------------------------------------------------------------- the cases pinned by the fixture
def _bench(name):
    return {"cfg1": scenes.config1, "cfg2": scenes.config2, "cfg3": scenes.config3, "cfg4": scenes.config4, "cfg5": scenes.config5,
            "head": lambda: scenes.head_scene(800, 800, 256, 10, textures=scenes.load_asset_textures())}[name]()


CASES = {
    **{name: (lambda name=name: _bench(name)) for name in ("cfg1", "cfg2", "cfg3", "cfg4", "cfg5", "head")},
    **{f"scatter-{s}": (lambda s=s: scatter_scene(500 + s, skew=(s % 2 == 0))) for s in range(4)},
    **{f"mesh-{s}": (lambda s=s: mesh_scene(900 + s, s % 3 == 0)) for s in range(4)},
    **{f"edge-{spp}{side}{kind}": (lambda spp=spp, side=side, kind=kind: tile_edge_scene(spp, side, kind))
       for spp, side, kind in ((1, "+", "sphere"), (3, "-", "mesh"), (8, "+", "mesh"), (24, "-", "sphere"))},
    "beyond-one-pixel": beyond_one_pixel_scene,
}


def record(run):
    """{case: {world: {applies, n_words, sha256, dead}}} with run(flat, cam, world) -> (applies, words, dead)."""
    out = {}
    for name, make in CASES.items():
        sc = make()
        flat = sc.flatten()
        out[name] = {}
        for world in WORLDS:
            applies, words, dead = run(flat, sc.camera, world)
            out[name][str(world)] = {"applies": applies, "n_words": int(len(words)), "sha256": digest(words), "dead": dead}
    return out


def test_masks_equal_the_recorded_ones(planner):
    with open(GOLDEN) as fh:
        want = json.load(fh)
    assert sorted(want) == sorted(CASES)

    def run(flat, cam, world):
        rc, applies, words, dead, _ = masks(planner, flat, cam, world)
        assert rc == abi.MI_OK
        return applies, words, dead

    got = record(run)
    for name in CASES:
        assert got[name] == want[name], name
    # what the cases are there for: dead tiles in the edge and jitter scenes, none where a Plane or ConvexVolume is
    assert all(want[n]["1"]["applies"] for n in CASES)
    assert sum(want["beyond-one-pixel"]["1"]["dead"]) > 0 and sum(want["edge-3-mesh"]["1"]["dead"]) > 0
    assert sum(want["mesh-0"]["1"]["dead"]) == 0 and sum(want["cfg2"]["1"]["dead"]) > 0


# ---------------------------------------------------------------------------------------------- where masking does not apply
def _small(cam_kw=None, objs=None, n_tri=3, n_sph=1):
    kw = dict(eyepoint=(0.0, 0.0, 2.0), view_dir=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), path_depth=3, path_samples=1,
              screen_width=100, screen_height=70, focal_length=0.7, focus_dist=4.0, lens_radius=0.0, aa_sample_count=4,
              max_trace_dist=100.0, gamma=2.0)
    kw.update(cam_kw or {})
    m = Lambertian(albedo=(0.5, 0.5, 0.5), emission=(1.0, 1.0, 1.0))
    if objs is None:
        objs = [Triangle((-0.5 + k, 0.0, -3.0), (0.5 + k, 0.0, -3.0), (k, 0.7, -3.0), m) for k in range(n_tri)]
        objs += [Sphere((1.0 + 0.5 * k, -1.0, -4.0), 0.3, m) for k in range(n_sph)]
    return Scene(Camera(**kw), objs)


NOT_APPLIED = {
    "orthographic": lambda: (_small({"projection_mode": abi.MI_PROJ_ORTHOGRAPHIC}), 0),
    "lens": lambda: (_small({"lens_radius": 0.05}), 0),
    "focus_dist 0": lambda: (_small({"focus_dist": 0.0}), 0),
    "focus_dist < 0": lambda: (_small({"focus_dist": -2.0}), 0),
    "MI_OPT_NO_TILE_MASKS": lambda: (_small(), abi.MI_OPT_NO_TILE_MASKS),
    "planes and volumes only": lambda: (_small(objs=[Plane((0.0, -1.0, 0.0), (0.0, 1.0, 0.0), Lambertian()),
                                                     ConvexVolume(Sphere((0.0, 0.0, -3.0), 1.0, Lambertian()), Isotropic(), 0.5)]), 0),
    "65 list entries": lambda: (_small(n_tri=60, n_sph=5), 0),
    "33 meshes": lambda: (_small(objs=_meshes(33)), 0),
    "near-singular basis": lambda: (_small({"up": (1e-7, 0.0, 1.0)}), 0),
}


def _meshes(n):
    from test_oracle_kat import cube_mesh
    from cs397raytracingsp22_amd import StaticMesh, cgmath
    return [StaticMesh(cube_mesh(-0.2, 0.2), Lambertian(), [None] * 5, cgmath.from_translation((0.5 * (k % 8) - 2.0, 0.5 * (k // 8) - 1.0, -5.0)))
            for k in range(n)]


@pytest.mark.parametrize("case", sorted(NOT_APPLIED))
def test_cases_where_masking_does_not_apply(planner, case):
    sc, flags = NOT_APPLIED[case]()
    for world in WORLDS:
        rc, applies, words, dead, _ = masks(planner, sc.flatten(), sc.camera, world, flags)
        assert rc == abi.MI_OK and not applies and len(words) == 0 and dead == [0] * world, (case, world)


def test_masking_applies_at_the_limits(planner):
    """64 list entries and 32 meshes are still masked: the cases above fail for the reason they name."""
    for sc in (_small(n_tri=60, n_sph=4), _small(objs=_meshes(32)), _small({"up": (1e-5, 0.0, 1.0)})):
        rc, applies, _, _, _ = masks(planner, sc.flatten(), sc.camera, 1)
        assert rc == abi.MI_OK and applies


# ---------------------------------------------------------------------------------------------- the grid and the masks' shape
@pytest.mark.parametrize("name", ["cfg1", "beyond-one-pixel", "edge-8+mesh", "mesh-1"])
def test_surplus_columns_and_the_partition(planner, name):
    """World 3 and 8 pad the row length to a coprime one: those columns hold no pixel, their tiles are dead with empty masks.
    The per-rank pixels and the grid equal dist.py's partition."""
    sc = CASES[name]()
    flat = sc.flatten()
    cam = sc.camera
    W, H = cam.screen_width, cam.screen_height
    tx_image, ty = -(-W // abi.MI_TILE), -(-H // abi.MI_TILE)
    for world in WORLDS:
        rc, applies, words, dead, pixels = masks(planner, flat, cam, world)
        assert rc == abi.MI_OK and applies
        stride, rows, n = dist.tile_grid(W, H, world)
        assert rows == ty and len(words) == 2 * n and stride >= tx_image
        lst, msh = words[:n].reshape(ty, stride), words[n:].reshape(ty, stride)
        assert (lst[:, tx_image:] == 0).all() and (msh[:, tx_image:] == np.uint64(DEAD)).all()
        assert sum(pixels) == W * H
        # the dead-sample count is the dead tiles' in-image pixels times spp
        dead_px = 0
        for t in range(n):
            x0, y0 = (t % stride) * abi.MI_TILE, (t // stride) * abi.MI_TILE
            if x0 < W and int(msh.ravel()[t]) >> 63:
                dead_px += min(abi.MI_TILE, W - x0) * min(abi.MI_TILE, H - y0)
        assert sum(dead) == dead_px * cam.aa_sample_count


@pytest.mark.parametrize("name", ["mesh-0", "mesh-3", "cfg5", "head"])
def test_no_dead_tile_beside_a_plane_or_volume(planner, name):
    sc = CASES[name]()
    assert any(isinstance(o, (Plane, ConvexVolume)) for o in sc.objects)
    for world in WORLDS:
        _, applies, words, dead, _ = masks(planner, sc.flatten(), sc.camera, world)
        n = len(words) // 2
        tx_image = -(-sc.camera.screen_width // abi.MI_TILE)
        msh = words[n:].reshape(-1, n // (-(-sc.camera.screen_height // abi.MI_TILE)))
        assert applies and not (msh[:, :tx_image] >> np.uint64(63)).any() and dead == [0] * world


# ---------------------------------------------------------------------------------------------- batch arithmetic
PER_PATH, PER_PATH_TS = 2 * 6 * 16 + 16, 8 * 8 + 8


def test_a_budget_below_one_sample_per_pixel_is_refused(planner):
    npix = 1024 * 40
    for two_stage in (False, True):
        per = PER_PATH + (PER_PATH_TS if two_stage else 0)
        rc, q = batch(planner, npix, 16, max_state_bytes=npix * per - 1, two_stage=two_stage)
        assert rc == abi.MI_ERR_INVALID and b"max_state_bytes" in q.err, q.err
        assert str(npix * per).encode() in q.err
        rc, q = batch(planner, npix, 16, max_state_bytes=npix * per, two_stage=two_stage)
        assert rc == abi.MI_OK and q.s_batch == 1


def test_no_budget_gives_at_least_one_sample(planner):
    rc, q = batch(planner, 1024 * 2040, 256, max_state_bytes=0, free_bytes=0)
    assert rc == abi.MI_OK and q.s_batch == 1
    rc, q = batch(planner, 1024 * 2040, 256, max_state_bytes=0, free_bytes=1000)
    assert rc == abi.MI_OK and q.s_batch == 1


@pytest.mark.parametrize("npix,spp,budget,free", [(1024 * 2040, 256, 0, 288 << 30), (1024 * 2040, 4096, 0, 288 << 30),
                                                  (1024 * 160, 16, 0, 288 << 30), (1024 * 2040, 1024, 1 << 40, 0),
                                                  (1024 * 7, 65535, 0, 1 << 50), (1024 * 255, 256, 5 << 30, 0)])
def test_batches_stay_within_the_path_cap_and_spp(planner, npix, spp, budget, free):
    for two_stage in (False, True):
        rc, q = batch(planner, npix, spp, max_state_bytes=budget, free_bytes=free, two_stage=two_stage)
        per = PER_PATH + (PER_PATH_TS if two_stage else 0)
        assert rc == abi.MI_OK
        assert 1 <= q.s_batch <= spp and npix * q.s_batch <= 1 << 31
        limit = min(1 << 31, budget // per if budget else int(free * 0.6 / per))
        assert q.s_batch == max(1, min(spp, limit // npix))
        blocks = -(-npix * q.s_batch // 256)
        assert q.region == (-(-blocks // 256) + 3) * 256 and q.cap == q.region * 256
        assert q.state_bytes == 6 * 16 * q.cap and q.samp_bytes == 16 * npix * q.s_batch and q.acc_bytes == 16 * npix
