"""Point-table rendering (mi_render_points / mi_render_points_device): lightmap baking with the rays made on the GPU, against the oracle.

The point tables are the oracle's first hits of tests/test_gpu_ray_table.py::fan_table rays (OracleScene.intersect): point = hitpoint +
1e-3 * normal, normal = RayHit.normal; misses are empty texels (zero normal), and every texel with (x + 2y) % 7 == 0 is forced empty, so
empty lanes sit inside live waves.  The oracle's side of sample s of pixel (x, y), built call by call:
    d = orc.scatter(Lambertian(0.5), p, n, frontface = 1, ray_dir = (0, 0, -1), seed, pixel = W*H + y*W + x, sample = s)[0]
    L = orc_shade(p, d, seed, y*W + x, s)
summed in f32 in sample order, / n in f32, orc.tonemap_pixel: oracle_image of the ray-table test with one more step in front.  Empty
texels are exactly zero.  Bars: those of tests/test_gpu_parity.py — per-channel RMS <= RMS_TOL, max |diff| <= 2e-5 * max(1, |ref|), u8
within 1 LSB.  Images are 75 x 41 (ragged in both tile directions); tables and oracle images are computed once per (scene, rows) and
shared, read-only, by the tests of this file."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Camera, Context, Lambertian, Scene, StaticMesh, abi, cgmath, dist as pdist, lightmap_texels, objload,
                                     scenes)
from cs397raytracingsp22_amd.tracing import ShadingMode

from test_gpu_ray_table import H, SCENES, SEED, W, assert_within_bars, bits, fan_table, same

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAT = Lambertian(albedo=(0.5, 0.5, 0.5))
ANY_DIR = (0.0, 0.0, -1.0)                          # Lambertian::scatter does not read the incoming ray
_cache = {}


def point_table(orc, name, rows):
    """(points, normals) [rows, H, W, 3] f32 of scene `name`: the first hits of the one-row fan (seed 21), offset by 1e-3 along the
    normal; rows == "aa" repeats them with the point jittered by at most 8.7e-4 (< 1e-3) per row, a position inside the texel's patch."""
    key = ("table", name, rows)
    if key not in _cache:
        if rows == "aa":
            p1, n1 = point_table(orc, name, 1)
            aa = SCENES[name][0]().camera.aa_sample_count
            jit = np.random.default_rng(77).uniform(-5e-4, 5e-4, (aa, H, W, 3)).astype(np.float32)
            live = n1.any(axis=-1)[..., None]
            p = np.where(live, p1 + jit, np.float32(0.0)).astype(np.float32)
            n = np.ascontiguousarray(np.broadcast_to(n1, p.shape))
        else:
            sc = SCENES[name][0]()
            o, d = fan_table(sc.camera, 1, 21)
            osc = orc.OracleScene(sc.flatten())
            p = np.zeros((1, H, W, 3), np.float32)
            n = np.zeros((1, H, W, 3), np.float32)
            for y in range(H):
                for x in range(W):
                    if (x + 2 * y) % 7 == 0:
                        continue                                                    # forced empty
                    rec = osc.intersect(o[0, y, x], d[0, y, x], 0.001, sc.camera.max_trace_dist, SEED, y * W + x, 0)
                    if rec.hit:
                        nn = np.float32(rec.normal[:])
                        p[0, y, x] = np.float32(rec.hitpoint[:]) + np.float32(1e-3) * nn
                        n[0, y, x] = nn
            osc.close()
        p.setflags(write=False)
        n.setflags(write=False)
        _cache[key] = (p, n)
    return _cache[key]


def directions(orc, name, rows):
    """The oracle's direction of every (row-or-sample, texel): [aa, H, W, 3] f32, zero where the texel is empty."""
    key = ("dirs", name, rows)
    if key not in _cache:
        p, n = point_table(orc, name, rows)
        aa = SCENES[name][0]().camera.aa_sample_count
        d = np.zeros((aa, H, W, 3), np.float32)
        for s in range(aa):
            row = s if p.shape[0] > 1 else 0
            for y in range(H):
                for x in range(W):
                    if n[row, y, x].any():
                        d[s, y, x] = orc.scatter(MAT, p[row, y, x], n[row, y, x], 1, ANY_DIR, SEED, W * H + y * W + x, s)[0]
        d.setflags(write=False)
        _cache[key] = d
    return _cache[key]


def reference(orc, name, rows):
    """(f32 mean, u8, empty [H, W] bool) of the oracle for the table of (name, rows)."""
    key = ("ref", name, rows)
    if key not in _cache:
        sc = SCENES[name][0]()
        p, n = point_table(orc, name, rows)
        d = directions(orc, name, rows)
        aa = sc.camera.aa_sample_count
        empty = ~n.any(axis=-1).any(axis=0)
        lib, osc, pod = orc.load(), orc.OracleScene(sc.flatten()), sc.camera.to_pod()
        fp = C.POINTER(C.c_float)
        samples = np.zeros((aa, H, W, 3), np.float32)                               # an empty texel shades nothing: exactly zero
        for s in range(aa):
            row = s if p.shape[0] > 1 else 0
            for y, x in zip(*np.nonzero(~empty)):
                rc = lib.orc_shade(osc._h, C.byref(pod), C.cast(p[row, y, x].ctypes.data, fp), C.cast(d[s, y, x].ctypes.data, fp),
                                   SEED, int(y * W + x), s, C.cast(samples[s, y, x].ctypes.data, fp))
                assert rc == 0
        osc.close()
        acc = np.zeros((H, W, 3), np.float32)
        for s in range(aa):
            acc = acc + samples[s]                              # final_color += shade_ray(..)  tracing.rs:238
        r32 = acc / np.float32(aa)                              # :241
        r8 = np.stack([orc.tonemap_pixel(px, sc.camera.gamma) for px in r32.reshape(-1, 3)]).reshape(H, W, 3)
        _cache[key] = (r32, r8, empty)
    return _cache[key]


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("rows", [1, "aa"])
@pytest.mark.parametrize("name", list(SCENES))
def test_against_the_oracle(gpu_ctx, orc, name, rows):
    sc = SCENES[name][0]()
    aa = sc.camera.aa_sample_count
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, rows)
    assert p.shape[0] == (1 if rows == 1 else aa)
    r32, r8, empty = reference(orc, name, rows)
    lit, share = int((r32.sum(axis=-1) > 0).sum()), float(empty.mean())
    print(f"{name} rows={rows}: {lit} lit reference pixels, {100 * share:.1f} % empty texels")
    assert lit >= 100 and 0.10 <= share <= 0.60                                   # the oracle's side alone: the case is not vacuous
    f32, u8, sig, st = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)
    assert st.samples == W * H * aa                                                # slots, empty texels included
    assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    g32, g8, none, _ = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=False)
    assert none is None and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    assert np.array_equal(bits(f32), bits(g32)) and np.array_equal(u8, g8)         # signatures on / off: the same image, bit for bit
    assert not bits(f32)[empty].any() and not sig[empty].any()                     # empty texels: +0.0 in every channel, signature 0
    assert np.array_equal(u8[empty], r8[empty]) and not r8[empty].any()            # and the tone-mapped zero
    assert_within_bars(f32, u8, r32, r8, f"{name} rows={rows}")


# ---------------------------------------------------------------- 2. equals a ray-table render of the same rays
@pytest.mark.parametrize("name", list(SCENES))
def test_equals_a_ray_table_render(gpu_ctx, orc, name):
    """render_points(P, N) against render_rays(P, D), D the oracle's directions: the same path stream and the same f32 operations
    (-ffp-contract=off), so the images agree to the bit wherever the kernel's direction has the oracle's bits."""
    sc = SCENES[name][0]()
    aa = sc.camera.aa_sample_count
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, 1)
    d = directions(orc, name, 1)
    empty = ~n.any(axis=-1)[0]
    pts = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)[:3]
    o = np.ascontiguousarray(np.broadcast_to(p, (aa, H, W, 3)))
    rays = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_sig=True)[:3]
    live = ~empty
    diff32 = int((bits(pts[0])[live] != bits(rays[0])[live]).any(axis=-1).sum())
    diffsig = int((pts[2][live] != rays[2][live]).sum())
    print(f"{name}: {diff32} of {int(live.sum())} live pixels differ in f32 bits, {diffsig} in signature")
    assert_within_bars(pts[0][live], pts[1][live], rays[0][live], rays[1][live], f"{name} points vs rays")
    assert diff32 == 0 and diffsig == 0 and np.array_equal(pts[1][live], rays[1][live])


# ---------------------------------------------------------------- 3. exactness across schedules
def device_render(ctx, cam, p, n, world, seed, flags=0, split=None, max_state_bytes=0):
    """The device form: every rank's tiles in turn into a gathered buffer, un-permute + tone map on the device, signatures un-permuted
    with the numpy mirror of the mapping.  split = k renders [0, k) and [k, aa) as two progressive calls with the accumulator copied out
    to the host and back in between."""
    import torch
    dev = torch.device("cuda:0")
    t_p, t_n = torch.from_numpy(np.array(p)).to(dev), torch.from_numpy(np.array(n)).to(dev)
    Wc, Hc = cam.screen_width, cam.screen_height
    padded = pdist.tiles_padded(Wc, Hc, world)
    gathered = torch.full((world, padded, pdist.TILE_PIXELS, 3), float("nan"), dtype=torch.float32, device=dev)
    gsig = torch.zeros((world, padded, pdist.TILE_PIXELS), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    samples = 0
    for r in range(world):
        kw = dict(seed=seed, rank=r, world=world, flags=flags, max_state_bytes=max_state_bytes)
        if split is None:
            st = ctx.render_points_device(cam, t_p.data_ptr(), t_n.data_ptr(), p.shape[0], gathered[r].data_ptr(), gsig[r].data_ptr(), **kw)
            samples += st.samples
        else:
            acc = torch.full((padded * pdist.TILE_PIXELS, 4), float("nan"), dtype=torch.float32, device=dev)
            st = ctx.render_points_device(cam, t_p.data_ptr(), t_n.data_ptr(), p.shape[0], None, gsig[r].data_ptr(), 0, split, acc.data_ptr(), **kw)
            samples += st.samples
            saved = acc.cpu()
            acc2 = saved.to(dev)                           # "another process": the sums travel through the host
            torch.cuda.synchronize(dev)
            st = ctx.render_points_device(cam, t_p.data_ptr(), t_n.data_ptr(), p.shape[0], gathered[r].data_ptr(), gsig[r].data_ptr(),
                                          split, cam.aa_sample_count, acc2.data_ptr(), **kw)
            samples += st.samples
    image = torch.empty((Hc, Wc, 3), dtype=torch.float32, device=dev)
    u8 = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=dev)
    ctx.unpermute_device(cam, world, gathered.data_ptr(), image.data_ptr())
    ctx.tonemap_device(cam, image.data_ptr(), u8.data_ptr())
    torch.cuda.synchronize(dev)
    assert not torch.isnan(gathered).any()                 # padding slots, pixels outside the image and empty texels are written as zeros
    r_of, idx = pdist.compact_index(Wc, Hc, world)
    sig = gsig.cpu().numpy().view(np.uint32).reshape(world, -1)[r_of, idx]
    assert samples == Wc * Hc * cam.aa_sample_count
    return image.cpu().numpy(), u8.cpu().numpy(), sig


@pytest.mark.parametrize("name", ["config2", "long_list", "head", "rare_top", "gv_mesh_top"])
def test_schedules_are_bit_identical(gpu_ctx, orc, name):
    sc = SCENES[name][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, "aa")
    base = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True)[:3]
    assert base[0].max() > 0 and len(np.unique(base[2])) > 100
    launches = gpu_ctx.last_pipeline_ms()["launches"]
    # one sample per batch: the budget of one sample of every padded pixel (208 B per path, 72 B more with a two-stage mesh)
    npix = pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS
    got = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True, max_state_bytes=npix * (2 * 6 * 16 + 16 + 72))[:3]
    assert gpu_ctx.last_pipeline_ms()["launches"] > launches
    assert same(got, base), "one sample per batch"
    for flags in (abi.MI_OPT_NO_LIST_TREE, abi.MI_OPT_REFERENCE_WALK, abi.MI_OPT_TWO_STAGE, abi.MI_OPT_NO_TILE_MASKS):
        got = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True, flags=flags)[:3]
        assert same(got, base), f"flags {flags}"
        assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    for world in (1, 2, 3):                                                        # world 1 is also: the host against the device entry point
        assert same(device_render(gpu_ctx, cam, p, n, world, SEED), base), f"world {world}"
    assert same(device_render(gpu_ctx, cam, p, n, 1, SEED, split=1), base), "progressive split [0, 1) + [1, aa)"
    assert same(device_render(gpu_ctx, cam, p, n, 2, SEED, split=1), base), "progressive, two ranks"


@pytest.mark.parametrize("name,rows", [("config4", 1), ("config5", "aa")])
def test_host_and_device_forms_give_the_same_bytes(gpu_ctx, orc, name, rows):
    sc = SCENES[name][0]()
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, rows)
    host = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)[:3]
    assert host[0].max() > 0
    assert same(device_render(gpu_ctx, sc.camera, p, n, 1, SEED), host)


# ---------------------------------------------------------------- 4. all-empty and edge shapes
def _small(sc, w, h, aa=4, depth=6):
    cam = sc.camera
    cam.screen_width, cam.screen_height, cam.aa_sample_count, cam.path_depth = w, h, aa, depth
    return sc


PROBE_P, PROBE_N = (0.3, 4.5, 0.5), (0.0, 1.0, 0.0)                                # a probe point under the Cornell box's ceiling light, facing it


def test_a_table_of_zero_normals_is_a_black_image(gpu_ctx):
    sc = SCENES["config2"][0]()
    gpu_ctx.upload(sc.flatten())
    p = np.random.default_rng(3).normal(size=(H, W, 3)).astype(np.float32)         # points of empty texels are not looked at
    n = np.zeros((H, W, 3), np.float32)
    n[::2, ::3] = -0.0                                                             # either sign of zero
    f32, u8, sig, st = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)     # MI_OK, or check() raises
    assert st.samples == W * H * sc.camera.aa_sample_count
    assert not bits(f32).any() and not u8.any() and not sig.any()
    counts = gpu_ctx.last_pipeline_counts()
    assert counts["dead_tile_samples"] == 0 and counts["segments"] == 0            # not one Scene::intersect_ray was evaluated
    for world in (1, 2):
        got = device_render(gpu_ctx, sc.camera, p[None], n[None], world, SEED)
        assert not bits(got[0]).any() and not got[1].any() and not got[2].any()


def test_one_pixel_image(gpu_ctx, orc):
    sc = _small(scenes.config1(), 1, 1)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    p, n = np.float32(PROBE_P).reshape(1, 1, 3), np.float32(PROBE_N).reshape(1, 1, 3)
    f32, u8, _, st = gpu_ctx.render_points(sc.camera, p, n, seed=SEED)
    assert st.samples == 4 and f32.shape == (1, 1, 3)
    osc = orc.OracleScene(flat)
    acc = np.zeros(3, np.float32)
    for s in range(4):
        d = orc.scatter(MAT, PROBE_P, PROBE_N, 1, ANY_DIR, SEED, 1 * 1 + 0, s)[0]
        acc = acc + osc.shade(sc.camera, PROBE_P, d, seed=SEED, pixel=0, sample=s)
    osc.close()
    ref = acc / np.float32(4)
    assert ref.sum() > 0
    assert float((np.abs(f32[0, 0].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()) <= 2e-5
    assert int(np.abs(u8[0, 0].astype(int) - orc.tonemap_pixel(ref, sc.camera.gamma).astype(int)).max()) <= 1


def test_a_row_whose_only_live_texel_is_the_last(gpu_ctx, orc):
    sc = _small(scenes.config1(), 33, 1)                                           # two tile columns, the second one pixel wide
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    p, n = np.zeros((1, 33, 3), np.float32), np.zeros((1, 33, 3), np.float32)
    p[0, 32], n[0, 32] = PROBE_P, PROBE_N
    f32, u8, sig, _ = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)
    assert not bits(f32)[0, :32].any() and not u8[0, :32].any() and not sig[0, :32].any()
    osc = orc.OracleScene(flat)
    acc = np.zeros(3, np.float32)
    for s in range(4):
        d = orc.scatter(MAT, PROBE_P, PROBE_N, 1, ANY_DIR, SEED, 33 * 1 + 32, s)[0]
        acc = acc + osc.shade(sc.camera, PROBE_P, d, seed=SEED, pixel=32, sample=s)
    osc.close()
    ref = acc / np.float32(4)
    assert ref.sum() > 0 and sig[0, 32] != 0
    assert float((np.abs(f32[0, 32].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()) <= 2e-5


def test_path_depth_zero_is_black(gpu_ctx, orc):
    sc = SCENES["config2"][0]()
    sc.camera.path_depth = 0
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, "config2", 1)
    f32, u8, sig, _ = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)
    assert not f32.any() and not u8.any() and not np.signbit(f32).any()
    g32, _, _, _ = gpu_ctx.render_points(sc.camera, p, n, seed=SEED)
    assert not g32.any()


# ---------------------------------------------------------------- 5. bad texels
@pytest.mark.parametrize("name", ["config1", "config2", "head"])
def test_bad_texels_do_not_disturb_their_neighbours(gpu_ctx, orc, name):
    """NaN and infinite points and normals at a handful of pixels: MI_OK, and every other pixel has exactly the bits of the clean render
    (a pixel's samples depend on nothing but its own texel and its own two streams; no address depends on the table's values)."""
    sc = SCENES[name][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, "aa")
    good = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True)[:3]
    nan, inf = np.float32("nan"), np.float32("inf")
    bad_n = [(nan, nan, nan), (inf, 0.0, 0.0), (0.0, -inf, 0.0), (nan, 0.0, 0.0), (0.0, 0.0, nan), (-inf, inf, -inf), (3e38, 3e38, -3e38),
             (1e-45, 0.0, 0.0), (0.0, nan, 0.0)]
    bad_p = [(nan, 0.0, 0.0), (inf, inf, inf), (0.0, -inf, 5.0), (3e38, 3.0, 6.6), (nan, nan, nan)]
    p2, n2 = np.array(p), np.array(n)
    mask = np.zeros((H, W), bool)
    pix = np.random.default_rng(2).choice(H * W, 60, replace=False)
    for k, q in enumerate(pix):
        y, x = divmod(int(q), W)
        s = k % cam.aa_sample_count if k % 3 else slice(None)                     # one row of the texel, or all of them
        if k % 4 == 3:
            p2[s, y, x] = bad_p[k % len(bad_p)]
            n2[s, y, x] = (0.0, 1.0, 0.0)                                         # (an empty texel's point would not be read at all)
        else:
            n2[s, y, x] = bad_n[k % len(bad_n)]
        mask[y, x] = True
    for y, x in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1)):                 # the image corners, next to the padded lanes
        n2[:, y, x] = (nan, nan, nan)
        p2[:, y, x] = (inf, nan, -inf)
        mask[y, x] = True
    got = gpu_ctx.render_points(cam, p2, n2, seed=SEED, want_sig=True)[:3]         # MI_OK, or check() raises
    keep = ~mask
    assert keep.sum() > 3000
    for a, b in zip(got, good):
        assert np.array_equal(bits(a)[keep], bits(b)[keep])
    again = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True)[:3]         # and the context is as good as before
    assert same(again, good)


# ---------------------------------------------------------------- 6. refusals
def test_refusals_launch_nothing(gpu_ctx, orc):
    lib = abi.load()
    sc = SCENES["config1"][0]()
    gpu_ctx.upload(sc.flatten())
    p, n = (np.array(a) for a in point_table(orc, "config1", "aa"))
    f32 = np.full((H, W, 3), -7.0, np.float32)
    h, pp, pn, pf = gpu_ctx._h, p.ctypes.data, n.ctypes.data, f32.ctypes.data
    nan = float("nan")

    def call(ctx=h, rows=4, pts=pp, nrm=pn, variant=0, rank=0, world=1, device=False, **cam_kw):
        cam = SCENES["config1"][0]().camera
        for k, v in cam_kw.items():
            setattr(cam, k, v)
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=SEED, rank=rank, world=world, variant=variant, want_signature=0, flags=0, max_state_bytes=0)
        if device:        # every refusal comes before a pointer is used: the host arrays stand in for device memory here
            rc = lib.mi_render_points_device(ctx, C.byref(pod), C.byref(opts), pts, nrm, rows, 0, cam.aa_sample_count, None, pf, None, None, None)
        else:
            rc = lib.mi_render_points(ctx, C.byref(pod), C.byref(opts), pts, nrm, rows, pf, None, None, None)
        msg = lib.mi_last_error().decode()
        assert rc == abi.MI_OK or len(msg) > 10, (rc, msg)
        return rc, msg

    assert call()[0] == abi.MI_OK and f32.max() > 0
    f32[:] = -7.0
    ms_before = gpu_ctx.last_kernel_ms()
    counts_before = gpu_ctx.last_pipeline_counts()
    for device in (False, True):
        kw = dict(device=device)
        rc, msg = call(path_samples=2, **kw)
        assert rc == abi.MI_ERR_UNSUPPORTED and "mi_shade_rays" in msg
        rc, msg = call(shading_mode=ShadingMode.Phong, **kw)
        assert rc == abi.MI_ERR_UNSUPPORTED and len(msg) > 10
        for variant in (abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_VOTED_DIAG, abi.MI_VARIANT_RECURSIVE, 2, 99):
            assert call(variant=variant, **kw)[0] == abi.MI_ERR_UNSUPPORTED, variant
        for bad in (dict(path_samples=0), dict(max_trace_dist=nan), dict(gamma=0.0), dict(gamma=nan), dict(screen_width=0),
                    dict(screen_width=40000), dict(aa_sample_count=0)):
            assert call(**bad, **kw)[0] == abi.MI_ERR_INVALID, bad
        for rows in (0, 2, 3, 5, 16):
            assert call(rows=rows, **kw)[0] == abi.MI_ERR_INVALID, rows
        rc, msg = call(pts=None, **kw)
        assert rc == abi.MI_ERR_INVALID and "mi_render_points" in msg
        assert call(nrm=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(ctx=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(rank=1, world=1, **kw)[0] == abi.MI_ERR_INVALID
    assert call(rank=0, world=2)[0] == abi.MI_ERR_INVALID                           # the host form renders a whole image
    assert np.all(f32 == -7.0)                                                      # nothing was written ...
    assert gpu_ctx.last_kernel_ms() == ms_before and gpu_ctx.last_pipeline_counts() == counts_before      # ... and nothing was launched
    fresh = Context(0)
    try:
        for device in (False, True):
            assert call(ctx=fresh._h, device=device)[0] == abi.MI_ERR_NO_SCENE
    finally:
        fresh.close()
    assert call()[0] == abi.MI_OK and f32.max() > 0                                 # the context is still good
    # a device-form range without an accumulator, and the other progressive rules of mi_render_samples_device
    import torch
    cam = sc.camera
    t_p, t_n = torch.from_numpy(p).to("cuda:0"), torch.from_numpy(n).to("cuda:0")
    acc = torch.zeros((pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS, 4), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for b, e, a, c in ((0, 2, None, None), (0, 2, None, out), (1, 4, None, out), (2, 2, acc, out), (3, 2, acc, out), (0, 5, acc, out),
                       (0, 4, acc, None), (0, 4, None, None)):
        with pytest.raises(abi.MiError) as ei:
            gpu_ctx.render_points_device(cam, t_p.data_ptr(), t_n.data_ptr(), 4, c.data_ptr() if c is not None else None, None, b, e,
                                         a.data_ptr() if a is not None else None)
        assert ei.value.code == abi.MI_ERR_INVALID and len(str(ei.value)) > 10, (b, e)
    with pytest.raises(ValueError):                                                 # and the Python mirror checks before any call
        gpu_ctx.render_points(cam, p[:2], n[:2])


# ---------------------------------------------------------------- 7. mi_render is untouched
def test_render_is_bit_identical_before_and_after_a_point_table_render(gpu_ctx, orc):
    sc = scenes.config2(240, 136, 16, 10)
    gpu_ctx.upload(sc.flatten())
    gpu_ctx.reserve(sc.camera)
    a32, a8, asig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    gpu_ctx.render(sc.camera, seed=1)
    dead = gpu_ctx.last_pipeline_counts()["dead_tile_samples"]
    assert dead > 0                                                                 # the camera render culls dead tiles ...
    small = SCENES["config2"][0]().camera
    p, n = point_table(orc, "config2", 1)
    t32, _, _, _ = gpu_ctx.render_points(small, p, n, seed=1)
    assert t32.max() > 0 and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0      # ... the table render does not
    b32, b8, bsig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    assert np.array_equal(bits(a32), bits(b32)) and np.array_equal(asig, bsig) and np.array_equal(a8, b8)
    c32, _, _, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=False)
    assert np.array_equal(bits(a32), bits(c32)) and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == dead


# ---------------------------------------------------------------- 8. end to end: a cube's lightmap in the Cornell box
def test_cube_lightmap_in_the_cornell_box(gpu_ctx, orc):
    with gzip.open(os.path.join(ROOT, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
        mesh = objload.load_obj_text(fh.read())[0]
    xf = cgmath.mul(cgmath.from_translation((0.2, 1.6, -0.3)), cgmath.from_angle_y(25.0), cgmath.from_scale(0.8))
    cube = StaticMesh(mesh, Lambertian(albedo=(0.7, 0.7, 0.7)), [None] * 5, xf)
    LW = LH = 32
    cam = Camera(screen_width=LW, screen_height=LH, aa_sample_count=16, path_depth=6, max_trace_dist=100.0, gamma=2.0)
    sc = Scene(cam, scenes.cornell_walls() + [cube])
    p, n, covered = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, LW, LH, transform=xf, offset=1e-3)
    assert 0.5 * LW * LH <= covered.sum() < LW * LH                                 # the atlas leaves texels no face covers
    u8 = sc.render_points(p, n, seed=SEED)                                          # the whole public path, a context of its own
    assert u8.shape == (LH, LW, 3) and not u8[~covered].any()
    up, down = covered & (n[..., 1] > 0.99), covered & (n[..., 1] < -0.99)          # the face under the ceiling light, the face over the floor
    assert up.sum() > 80 and down.sum() > 80
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    f32, g8, sig, st = gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True)
    assert np.array_equal(g8, u8) and st.samples == LW * LH * 16
    assert not bits(f32)[~covered].any() and not sig[~covered].any()
    print(f"cube lightmap: mean radiance gathered by the top face {f32[up].mean():.3f}, by the bottom face {f32[down].mean():.3f}")
    assert f32[up].mean() > 2.0 * f32[down].mean() > 0.0
    # against the oracle, texel by texel
    osc = orc.OracleScene(flat)
    acc = np.zeros((LH, LW, 3), np.float32)
    for s in range(16):
        for y, x in zip(*np.nonzero(covered)):
            d = orc.scatter(MAT, p[y, x], n[y, x], 1, ANY_DIR, SEED, LW * LH + y * LW + x, s)[0]
            acc[y, x] = acc[y, x] + osc.shade(cam, p[y, x], d, seed=SEED, pixel=y * LW + x, sample=s)
    osc.close()
    r32 = acc / np.float32(16)
    r8 = np.stack([orc.tonemap_pixel(px, cam.gamma) for px in r32.reshape(-1, 3)]).reshape(LH, LW, 3)
    assert_within_bars(f32, u8, r32, r8, "cube lightmap")
