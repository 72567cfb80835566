"""Directional lightmaps on the GPU: mi_render_points_sh / _device / mi_bake_lightmap_sh against the oracle's own samples, and
mi_lightmap_finish_sh / mi_lightmap_sh_eval against their numpy definitions.

Bake: scenes, point tables and directions are those of tests/test_gpu_point_table.py (75 x 41, aa = 4, every (x + 2y) % 7 == 0 texel
empty).  The oracle's side of sample s of texel (x, y):
    d = orc.scatter(Lambertian, p, n, 1, any dir, seed, W*H + y*W + x, s)[0]        (sample_hemisphere, materials.rs:171-178)
    L = orc_shade(p, d, seed, y*W + x, s)
and the SH reference is the float64 projection ref_k,c = (2 pi / S) sum_s L_s,c Y_k(d_s / |d_s|) over the rows whose normal is not
zero, with the bar of tests/test_gpu_probes.py: |gpu - ref| <= 2e-5 * max(1, mass), mass the same sum of absolute values.  c_0 must equal
mean * 2 pi * Y_0 within 4 * 2^-23 of that scale (two roundings of the same sum).
Finish and evaluation: BIT-EQUALITY with the helpers, derived as in tests/test_gpu_lightmap_finish.py: no fused multiply-add, every
operation one of + - * /, sqrtf, fabsf, fmaxf, a comparison or an exact conversion, in a fixed order per texel on both sides."""
import ctypes as C

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Camera, Context, Lambertian, Scene, StaticMesh, abi, cgmath, dist as pdist, lightmap_finish,
                                     lightmap_finish_sh, lightmap_sh_eval, scenes, sh9_basis)
from cs397raytracingsp22_amd.tracing import ShadingMode, mesh_pod

import finish_batteries as fb
from finish_batteries import INF
from test_gpu_point_table import ANY_DIR, MAT, directions, point_table
from test_gpu_ray_table import H, SCENES, SEED, W, bits, same
from test_lightmap_sh_host import BATTERIES, _records_and_normals, sh_records

pytestmark = pytest.mark.gpu

TWO_PI = 2.0 * np.pi
Y0 = 0.28209479177387814
_cache = {}


# ---------------------------------------------------------------- the oracle's side
def oracle_samples(orc, sc, p, n, d=None, seed=SEED):
    """(d, L) [aa, h, w, 3] f32: the oracle's direction and radiance of every sample of the table (p, n) [rows, h, w, 3]; both zero for
    a row whose normal is zero.  `d`: directions already known."""
    cam = sc.camera
    aa, h, w = cam.aa_sample_count, cam.screen_height, cam.screen_width
    assert p.shape[1:] == (h, w, 3) and n.shape == p.shape
    lib, osc, pod = orc.load(), orc.OracleScene(sc.flatten()), cam.to_pod()
    fp = C.POINTER(C.c_float)
    known = d is not None
    d = np.array(d) if known else np.zeros((aa, h, w, 3), np.float32)
    L = np.zeros((aa, h, w, 3), np.float32)
    for s in range(aa):
        row = s if p.shape[0] > 1 else 0
        for y, x in zip(*np.nonzero(n[row].any(axis=-1))):
            if not known:
                d[s, y, x] = orc.scatter(MAT, p[row, y, x], n[row, y, x], 1, ANY_DIR, seed, w * h + int(y) * w + int(x), s)[0]
            rc = lib.orc_shade(osc._h, C.byref(pod), C.cast(p[row, y, x].ctypes.data, fp), C.cast(d[s, y, x].ctypes.data, fp),
                               seed, int(y) * w + int(x), s, C.cast(L[s, y, x].ctypes.data, fp))
            assert rc == 0
    osc.close()
    return d, L


def project(d, L, n):
    """(ref, mass) [h, w, 9, 3] float64: (2 pi / S) sum over the rows with a non-zero normal of L Y_k(d / |d|), and its absolute mass"""
    S = d.shape[0]
    live = np.broadcast_to(n.any(axis=-1), d.shape[:3])                             # [S, h, w]: one row serves every sample
    safe = np.where(live[..., None], d.astype(np.float64), np.float64([0.0, 1.0, 0.0]))
    Y = np.where(live[..., None], sh9_basis(safe), 0.0)                             # [S, h, w, 9]
    L64 = np.where(live[..., None], L.astype(np.float64), 0.0)
    ref = (TWO_PI / S) * (Y[..., :, None] * L64[..., None, :]).sum(axis=0)
    mass = (TWO_PI / S) * (np.abs(Y)[..., :, None] * np.abs(L64)[..., None, :]).sum(axis=0)
    return ref, mass


def sh_ratio(sh, ref, mass):
    assert np.isfinite(ref).all() and np.isfinite(sh).all()
    return float((np.abs(sh.astype(np.float64) - ref) / np.maximum(1.0, mass)).max())


def reference(orc, name, rows):
    """The oracle's SH projection for the table of (name, rows): (ref, mass), computed once and read-only"""
    key = (name, rows)
    if key not in _cache:
        sc = SCENES[name][0]()
        p, n = point_table(orc, name, rows)
        d, L = oracle_samples(orc, sc, p, n, d=directions(orc, name, rows))
        ref, mass = project(d, L, n)
        ref.setflags(write=False)
        mass.setflags(write=False)
        _cache[key] = (ref, mass)
    return _cache[key]


# ---------------------------------------------------------------- 1. the plain outputs are render_points'
@pytest.mark.parametrize("rows", [1, "aa"])
@pytest.mark.parametrize("name", ["config2", "head"])
def test_plain_outputs_are_render_points_bits(gpu_ctx, orc, name, rows):
    sc = SCENES[name][0]()
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, rows)
    plain = gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)[:3]
    assert plain[0].max() > 0 and gpu_ctx.last_reduce_psh_ms() == 0.0
    sh, f32, u8, sig, st = gpu_ctx.render_points_sh(sc.camera, p, n, seed=SEED, want_sig=True)
    assert gpu_ctx.last_reduce_psh_ms() > 0.0 and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    assert st.samples == W * H * sc.camera.aa_sample_count and sh.shape == (H, W, 9, 3)
    assert same((f32, u8, sig), plain)
    sh2, g32, g8, none, _ = gpu_ctx.render_points_sh(sc.camera, p, n, seed=SEED, want_sig=False)
    assert none is None and same((sh2, g32, g8), (sh, f32, u8))                    # signatures on / off
    empty = ~n.any(axis=-1).any(axis=0)
    assert empty.sum() > 300 and not bits(sh)[empty].any()                         # 27 x +0.0
    assert np.abs(sh[~empty][:, 1:, :]).max() > 0.1                                 # directional content


# ---------------------------------------------------------------- 2. the SH against the f64 projection of the oracle's samples
@pytest.mark.parametrize("name,rows", [(name, 1) for name in SCENES] + [("config2", "aa"), ("head", "aa")])
def test_sh_against_the_f64_projection(gpu_ctx, orc, name, rows):
    sc = SCENES[name][0]()
    p, n = point_table(orc, name, rows)
    ref, mass = reference(orc, name, rows)
    lit = int((mass.sum(axis=(-1, -2)) > 0).sum())
    print(f"{name} rows={rows}: {lit} texels with a non-zero mass")
    assert lit >= 100                                                              # the oracle's side alone: the case is not vacuous
    gpu_ctx.upload(sc.flatten())
    sh, f32, _, _, _ = gpu_ctx.render_points_sh(sc.camera, p, n, seed=SEED)
    ratio = sh_ratio(sh, ref, mass)
    c0 = np.abs(sh[:, :, 0, :].astype(np.float64) - f32.astype(np.float64) * (TWO_PI * Y0)) / np.maximum(1.0, mass[:, :, 0, :])
    print(f"{name} rows={rows}: max |sh - ref| / max(1, mass) = {ratio:.3e} (bar 2e-5); max |c_0 - mean 2 pi Y_0| / max(1, mass) = "
          f"{float(c0.max()) * 2 ** 23:.2f} ulp (bar 4); largest |coefficient| {float(np.abs(ref).max()):.3f}")
    assert ratio <= 2e-5
    assert float(c0.max()) <= 4 * 2.0 ** -23


# ---------------------------------------------------------------- 3. exactness across schedules
def device_render(ctx, cam, p, n, world, seed, flags=0, split=None, max_state_bytes=0, with_sh=True):
    """The device form: every rank's tiles in turn into gathered buffers (pre-filled with NaN).  split = k renders [0, k) and [k, aa) as
    two progressive calls with BOTH accumulators (the float4 sums and the SH records) copied out to the host and back in between.
    Returns (sh or None, f32, u8, sig)."""
    import torch
    dev = torch.device("cuda:0")
    t_p, t_n = torch.from_numpy(np.array(p)).to(dev), torch.from_numpy(np.array(n)).to(dev)
    Wc, Hc = cam.screen_width, cam.screen_height
    padded = pdist.tiles_padded(Wc, Hc, world)
    nan = float("nan")
    gathered = torch.full((world, padded, pdist.TILE_PIXELS, 3), nan, dtype=torch.float32, device=dev)
    gsh = torch.full((world, padded, pdist.TILE_PIXELS, 27), nan, dtype=torch.float32, device=dev)
    gsig = torch.zeros((world, padded, pdist.TILE_PIXELS), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    samples = 0
    for r in range(world):
        kw = dict(seed=seed, rank=r, world=world, flags=flags, max_state_bytes=max_state_bytes)
        tab = (t_p.data_ptr(), t_n.data_ptr(), p.shape[0])
        psh = gsh[r].data_ptr() if with_sh else None
        if split is None:
            samples += ctx.render_points_sh_device(cam, *tab, psh, gathered[r].data_ptr(), gsig[r].data_ptr(), **kw).samples
        else:
            acc = torch.full((padded * pdist.TILE_PIXELS, 4), nan, dtype=torch.float32, device=dev)
            samples += ctx.render_points_sh_device(cam, *tab, psh, None, gsig[r].data_ptr(), 0, split, acc.data_ptr(), **kw).samples
            saved, saved_sh = acc.cpu(), gsh[r].cpu()
            gsh[r] = nan
            acc2, sh2 = saved.to(dev), saved_sh.to(dev)     # "another process": both sums travel through the host
            torch.cuda.synchronize(dev)
            samples += ctx.render_points_sh_device(cam, *tab, sh2.data_ptr() if with_sh else None, gathered[r].data_ptr(),
                                                   gsig[r].data_ptr(), split, cam.aa_sample_count, acc2.data_ptr(), **kw).samples
            gsh[r] = sh2
    image = torch.empty((Hc, Wc, 3), dtype=torch.float32, device=dev)
    u8 = torch.empty((Hc, Wc, 3), dtype=torch.uint8, device=dev)
    ctx.unpermute_device(cam, world, gathered.data_ptr(), image.data_ptr())
    ctx.tonemap_device(cam, image.data_ptr(), u8.data_ptr())
    torch.cuda.synchronize(dev)
    assert not torch.isnan(gathered).any()
    r_of, idx = pdist.compact_index(Wc, Hc, world)
    sig = gsig.cpu().numpy().view(np.uint32).reshape(world, -1)[r_of, idx]
    assert samples == Wc * Hc * cam.aa_sample_count
    sh = None
    if with_sh:
        assert not torch.isnan(gsh).any()                   # padding slots are written, and no sum started from what the buffer held
        flat = gsh.cpu().numpy().reshape(world, -1, 27)
        inside = np.zeros(flat.shape[:2], bool)
        inside[r_of, idx] = True
        assert not flat.view(np.uint32)[~inside].any()      # +0.0 in every slot that is no texel
        sh = flat[r_of, idx].reshape(Hc, Wc, 9, 3)
    else:
        assert torch.isnan(gsh).all()                       # NULL: not touched
    return sh, image.cpu().numpy(), u8.cpu().numpy(), sig


@pytest.mark.parametrize("name", ["config2", "head", "gv_mesh_top"])
def test_schedules_are_bit_identical(gpu_ctx, orc, name):
    sc = SCENES[name][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, name, "aa")
    base = gpu_ctx.render_points_sh(cam, p, n, seed=SEED, want_sig=True)[:4]
    assert base[1].max() > 0 and np.abs(base[0][:, :, 1:, :]).max() > 0.1
    one = device_render(gpu_ctx, cam, p, n, 1, SEED)                                # one batch; also the host against the device entry point
    launches = gpu_ctx.last_pipeline_ms()["launches"]
    assert same(one, base), "world 1"
    npix = pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS                          # one sample per batch (208 B per path, 72 B more with a two-stage mesh)
    got = device_render(gpu_ctx, cam, p, n, 1, SEED, max_state_bytes=npix * (2 * 6 * 16 + 16 + 72))
    assert gpu_ctx.last_pipeline_ms()["launches"] > launches
    assert same(got, base), "one sample per batch"
    for world in (2, 3):
        assert same(device_render(gpu_ctx, cam, p, n, world, SEED), base), f"world {world}"
    for split in range(1, cam.aa_sample_count):
        assert same(device_render(gpu_ctx, cam, p, n, 1, SEED, split=split), base), f"progressive split at {split}"
    assert same(device_render(gpu_ctx, cam, p, n, 2, SEED, split=1), base), "progressive, two ranks"
    for flags in (abi.MI_OPT_TWO_STAGE, abi.MI_OPT_REFERENCE_WALK, abi.MI_OPT_NO_FINAL_CULL):
        assert same(device_render(gpu_ctx, cam, p, n, 1, SEED, flags=flags), base), f"flags {flags}"


def test_a_null_sh_buffer_is_render_points_device(gpu_ctx, orc):
    sc = SCENES["config2"][0]()
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, "config2", "aa")
    full = device_render(gpu_ctx, sc.camera, p, n, 1, SEED)
    assert gpu_ctx.last_reduce_psh_ms() > 0.0
    plain = device_render(gpu_ctx, sc.camera, p, n, 1, SEED, with_sh=False)
    assert plain[0] is None and same(plain[1:], full[1:]) and gpu_ctx.last_reduce_psh_ms() == 0.0
    assert same(plain[1:], gpu_ctx.render_points(sc.camera, p, n, seed=SEED, want_sig=True)[:3])


# ---------------------------------------------------------------- 4. small and edge shapes
def _small(w, h, aa=4, depth=6):
    sc = scenes.config1()
    cam = sc.camera
    cam.screen_width, cam.screen_height, cam.aa_sample_count, cam.path_depth = w, h, aa, depth
    return sc


PROBE_P, PROBE_N = (0.3, 4.5, 0.5), (0.0, 1.0, 0.0)                                # under the Cornell box's ceiling light, facing it


def _check_small(gpu_ctx, orc, sc, p, n, what):
    """a whole small table against the oracle: the SH under the bar; returns the GPU's outputs"""
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    sh, f32, u8, sig, st = gpu_ctx.render_points_sh(cam, p, n, seed=SEED, want_sig=True)
    assert st.samples == cam.screen_width * cam.screen_height * cam.aa_sample_count
    P4, N4 = (t if t.ndim == 4 else t[None] for t in (p, n))
    d, L = oracle_samples(orc, sc, P4, N4)
    ref, mass = project(d, L, N4)
    assert mass.sum() > 0, what
    ratio = sh_ratio(sh, ref, mass)
    print(f"{what}: SH ratio {ratio:.3e}")
    assert ratio <= 2e-5, what
    assert same((f32, u8, sig), gpu_ctx.render_points(cam, p, n, seed=SEED, want_sig=True)[:3]), what
    return sh, f32, u8, sig


def _line(count, axis):
    """`count` points under the light along x, as a [1, count, 3] (axis 1) or [count, 1, 3] (axis 0) table"""
    p = np.zeros((count, 3), np.float32)
    p[:, 0] = np.linspace(-2.0, 2.0, count)
    p[:, 1] = 4.5
    n = np.tile(np.float32(PROBE_N), (count, 1))
    shape = (1, count, 3) if axis == 1 else (count, 1, 3)
    return p.reshape(shape), n.reshape(shape)


def test_one_texel_image(gpu_ctx, orc):
    sh, _, _, _ = _check_small(gpu_ctx, orc, _small(1, 1), np.float32(PROBE_P).reshape(1, 1, 3), np.float32(PROBE_N).reshape(1, 1, 3), "1 x 1")
    assert sh.shape == (1, 1, 9, 3) and sh[0, 0, 1].min() > 0                       # the light is overhead: c_1 (y) is positive


@pytest.mark.parametrize("w,h", [(33, 1), (1, 33)])
def test_a_second_tile_one_texel_wide(gpu_ctx, orc, w, h):
    p, n = _line(33, 1 if h == 1 else 0)
    sc = _small(w, h)
    got = _check_small(gpu_ctx, orc, sc, p, n, f"{w} x {h}")
    assert np.abs(got[0].reshape(33, 9, 3)[32]).max() > 0
    assert same(device_render(gpu_ctx, sc.camera, p[None], n[None], 2, SEED), got)  # one tile per rank


def test_an_all_empty_table_is_all_positive_zero(gpu_ctx):
    sc = SCENES["config2"][0]()
    gpu_ctx.upload(sc.flatten())
    p = np.random.default_rng(3).normal(size=(H, W, 3)).astype(np.float32)
    n = np.zeros((H, W, 3), np.float32)
    n[::2, ::3] = -0.0
    sh, f32, u8, sig, _ = gpu_ctx.render_points_sh(sc.camera, p, n, seed=SEED, want_sig=True)        # MI_OK, or check() raises
    assert not bits(sh).any() and not bits(f32).any() and not u8.any() and not sig.any()
    assert gpu_ctx.last_pipeline_counts()["segments"] == 0
    got = device_render(gpu_ctx, sc.camera, p[None], n[None], 2, SEED)
    assert not bits(got[0]).any() and not bits(got[1]).any()


def test_a_row_whose_only_live_texel_is_the_last(gpu_ctx, orc):
    p, n = _line(33, 1)
    n = n.copy()
    n[0, :32] = 0.0
    sh, f32, _, _ = _check_small(gpu_ctx, orc, _small(33, 1), p, n, "only the last texel")
    assert not bits(sh)[0, :32].any() and np.abs(sh[0, 32]).max() > 0 and f32[0, 32].sum() > 0


def test_a_jittered_table_with_some_empty_rows(gpu_ctx, orc):
    """Texel (1, 0) has rows 0 and 2 empty, texel (3, 0) has only row 3 live: the sums are those over the live rows, the scale stays
    2 pi / S, and the empty rows bring no NaN."""
    aa = 4
    p1, n1 = _line(5, 1)
    p = np.ascontiguousarray(np.broadcast_to(p1, (aa, 1, 5, 3))) + np.random.default_rng(9).uniform(-5e-4, 5e-4, (aa, 1, 5, 3)).astype(np.float32)
    n = np.array(np.broadcast_to(n1, (aa, 1, 5, 3)))
    n[0, 0, 1] = n[2, 0, 1] = 0.0
    n[:3, 0, 3] = -0.0
    sh, f32, _, _ = _check_small(gpu_ctx, orc, _small(5, 1, aa=aa), p, n, "partly empty rows")
    assert np.isfinite(sh).all() and np.abs(sh[0, 1]).max() > 0 and np.abs(sh[0, 3]).max() > 0


def test_path_depth_zero_is_all_positive_zero(gpu_ctx, orc):
    sc = SCENES["config2"][0]()
    sc.camera.path_depth = 0
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, "config2", 1)
    sh, f32, u8, _, _ = gpu_ctx.render_points_sh(sc.camera, p, n, seed=SEED)
    assert not bits(sh).any() and not bits(f32).any() and not u8.any()
    assert not bits(device_render(gpu_ctx, sc.camera, p, n, 1, SEED)[0]).any()


# ---------------------------------------------------------------- 5. non-finite input
def test_bad_texels_do_not_disturb_their_neighbours(gpu_ctx, orc):
    sc = SCENES["config2"][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    p, n = point_table(orc, "config2", "aa")
    good = gpu_ctx.render_points_sh(cam, p, n, seed=SEED, want_sig=True)[:4]
    nan, inf = np.float32("nan"), np.float32("inf")
    bad = [(nan, 0.0, 0.0), (inf, inf, inf), (0.0, -inf, 5.0), (3e38, 3.0, 6.6), (nan, nan, nan), (-3e38, 3e38, 3e38), (0.0, nan, inf)]
    p2, n2 = np.array(p), np.array(n)
    mask = np.zeros((H, W), bool)
    for k, q in enumerate(np.random.default_rng(2).choice(H * W, 60, replace=False)):
        y, x = divmod(int(q), W)
        (p2 if k % 2 else n2)[k % cam.aa_sample_count if k % 3 else slice(None), y, x] = bad[k % len(bad)]      # a point or a normal, one row or all
        mask[y, x] = True
    for y, x in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1)):                 # the image corners, next to the padded lanes
        n2[:, y, x] = (inf, nan, -inf)
        mask[y, x] = True
    got = gpu_ctx.render_points_sh(cam, p2, n2, seed=SEED, want_sig=True)[:4]      # MI_OK, or check() raises
    keep = ~mask
    assert keep.sum() > 3000
    for a, b in zip(got, good):
        assert np.array_equal(bits(a)[keep], bits(b)[keep])
    assert same(gpu_ctx.render_points_sh(cam, p, n, seed=SEED, want_sig=True)[:4], good)


# ---------------------------------------------------------------- 6. the bake is the table and the render
def cube_bake(gpu_ctx):
    """The cube in the Cornell box, as test_cube_lightmap_in_the_cornell_box sets it up: (sh, f32, u8, sig, points, normals, scene, cube)"""
    if "bake" not in _cache:
        xf = cgmath.mul(cgmath.from_translation((0.2, 1.6, -0.3)), cgmath.from_angle_y(25.0), cgmath.from_scale(0.8))
        cube = StaticMesh(fb.cube_mesh(), Lambertian(albedo=(0.7, 0.7, 0.7)), [None] * 5, xf)
        cam = Camera(screen_width=32, screen_height=32, aa_sample_count=16, path_depth=6, max_trace_dist=100.0, gamma=2.0)
        sc = Scene(cam, scenes.cornell_walls() + [cube])
        gpu_ctx.upload(sc.flatten())
        sh, f32, u8, sig, tri, st = gpu_ctx.bake_lightmap_sh(cam, cube, jitter=True, offset=1e-3, seed=SEED, want_sig=True, want_triangle=True)
        assert st.samples == 32 * 32 * 16 and tri.shape == (16, 32, 32)
        _cache["bake"] = (sh, f32, u8, sig, tri, sc, cube)
    return _cache["bake"]


def test_bake_is_the_table_and_the_render(gpu_ctx):
    sh, f32, u8, sig, tri, sc, cube = cube_bake(gpu_ctx)
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    p, n, t = gpu_ctx.lightmap_texels(cube, 32, 32, rows=16, jitter=True, seed=SEED, offset=1e-3)
    assert np.array_equal(t, tri)
    assert same(gpu_ctx.render_points_sh(cam, p, n, seed=SEED, want_sig=True)[:4], (sh, f32, u8, sig))
    assert same(gpu_ctx.bake_lightmap(cam, cube, jitter=True, offset=1e-3, seed=SEED, want_sig=True)[:3], (f32, u8, sig))
    assert gpu_ctx.last_reduce_psh_ms() == 0.0
    sh1, m1, _, _, _, _ = gpu_ctx.bake_lightmap_sh(cam, cube, jitter=False, offset=1e-3, seed=SEED)
    p1, n1, _ = gpu_ctx.lightmap_texels(cube, 32, 32, rows=1, offset=1e-3)
    assert same(gpu_ctx.render_points_sh(cam, p1, n1, seed=SEED)[:2], (sh1, m1))
    # the Scene path: a context of its own
    got = sc.bake_lightmap(cube, 32, 32, 16, jitter=True, offset=1e-3, seed=SEED, directional=True)
    assert same(got, (sh, f32))
    params = dict(levels=2, normal_power_log2=5, sigma_plane=0.1, reach=0.5, sigma_color=8.0, dilate=2)
    fsh, fmean, valid = sc.bake_lightmap(cube, 32, 32, 16, jitter=True, offset=1e-3, seed=SEED, directional=True, finish=params)
    want, want_valid = lightmap_finish_sh(sh, p1[0], n1[0], **params)
    assert np.array_equal(bits(fsh), bits(want)) and np.array_equal(valid, want_valid)
    assert np.array_equal(bits(fmean), bits(lightmap_finish(f32, p1[0], n1[0], **params)[0]))


# ---------------------------------------------------------------- 7. the finish
_ref = {}


def finish_reference(name, sh, P, N, params):
    key = (name, tuple(sorted(params.items())))
    if key not in _ref:
        out, valid = lightmap_finish_sh(sh, P, N, **params)
        out.setflags(write=False)
        valid.setflags(write=False)
        _ref[key] = (out, valid)
    return _ref[key]


def assert_equals_helper(ctx, name, sh, P, N, params):
    want, want_valid = finish_reference(name, sh, P, N, params)
    out, valid = ctx.lightmap_finish_sh(sh, P, N, **params)
    wrong = int((bits(out) != bits(want)).any(axis=(-1, -2)).sum())
    print(f"{name} {params}: {int(want_valid.sum())} of {want_valid.size} texels valid, {wrong} texels differ in bits")
    assert np.array_equal(valid, want_valid), name
    assert wrong == 0, name


def _ragged(Wr, Hr, levels=4, dilate=2):
    name, img, P, N, params = fb.ragged_battery(Wr, Hr, levels=levels, dilate=dilate)
    return name, sh_records(img), P, N, params


def test_every_battery_has_the_helpers_bits(gpu_ctx):
    for name, sh, P, N, params in BATTERIES:
        assert_equals_helper(gpu_ctx, name, sh, P, N, params)
        assert_equals_helper(gpu_ctx, name, sh, P, N, dict(params, sigma_color=INF))
    for name, img, P, N, params in fb.limiting_batteries():                         # the masked copy, 1 x 1, an all-empty table
        assert_equals_helper(gpu_ctx, name, sh_records(img), P, N, params)


@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5])
def test_each_level_count_singly(gpu_ctx, levels):
    name, sh, P, N, params = BATTERIES[1]                                           # the noisy cube at 75 x 41
    assert_equals_helper(gpu_ctx, name, sh, P, N, dict(params, levels=levels, dilate=0))
    assert_equals_helper(gpu_ctx, *_ragged(65, 33, levels=levels, dilate=0))


@pytest.mark.parametrize("Wr", [31, 32, 33, 65])
def test_tile_edges(gpu_ctx, Wr):
    assert_equals_helper(gpu_ctx, *_ragged(Wr, 33))


def device_finish(ctx, sh, P, N, params, want_valid=True, stream=None, three=False):
    """mi_lightmap_finish_sh_device, or with `three` mi_lightmap_finish_device on a [H, W, 3] image"""
    import torch
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.array(a)).to(dev) for a in (sh, P, N)]
    out = torch.full(sh.shape, -7.0, dtype=torch.float32, device=dev)
    valid = torch.full(sh.shape[:2], 9, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    call = ctx.lightmap_finish_device if three else ctx.lightmap_finish_sh_device
    call(sh.shape[1], sh.shape[0], t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), out.data_ptr(), valid.data_ptr() if want_valid else None,
         stream=stream.cuda_stream if stream is not None else None, **params)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(dev)
    return out.cpu().numpy(), valid.cpu().numpy()


def test_device_form_and_the_two_identities(gpu_ctx):
    import torch
    name, sh, P, N, params = BATTERIES[1]
    want, want_valid = finish_reference(name, sh, P, N, params)
    first, first_valid = device_finish(gpu_ctx, sh, P, N, params)
    assert np.array_equal(bits(first), bits(want)) and np.array_equal(first_valid, want_valid.astype(np.uint8))
    assert gpu_ctx.last_kernel_ms() > 0.0
    again, again_valid = device_finish(gpu_ctx, sh, P, N, params, stream=torch.cuda.Stream(device="cuda:0"))
    assert np.array_equal(bits(again), bits(first)) and np.array_equal(again_valid, first_valid)
    small = BATTERIES[-1]                                                           # a smaller image after a larger one
    out, valid = device_finish(gpu_ctx, *small[1:])
    assert np.array_equal(bits(out), bits(finish_reference(*small)[0]))
    out, untouched = device_finish(gpu_ctx, sh, P, N, params, want_valid=False)
    assert np.array_equal(bits(out), bits(first)) and (untouched == 9).all()
    # between device calls: plane 0 against mi_lightmap_finish_device, and every plane without the colour weight
    plane0, valid0 = device_finish(gpu_ctx, np.ascontiguousarray(sh[:, :, 0, :]), P, N, params, three=True)
    assert np.array_equal(bits(first[:, :, 0, :]), bits(plane0)) and np.array_equal(first_valid, valid0)
    assert not np.array_equal(bits(first[:, :, 1, :]), bits(plane0))
    open_params = dict(params, sigma_color=INF)
    every, _ = device_finish(gpu_ctx, sh, P, N, open_params)
    for k in range(9):
        plane, _ = device_finish(gpu_ctx, np.ascontiguousarray(sh[:, :, k, :]), P, N, open_params, three=True)
        assert np.array_equal(bits(every[:, :, k, :]), bits(plane)), k


def test_device_form_refuses_an_overlapping_output(gpu_ctx):
    import torch
    dev = torch.device("cuda:0")
    Wd, Hd = 16, 8
    rec, tab = Hd * Wd * 108, Hd * Wd * 12
    buf = torch.full(((2 * rec + 2 * tab) // 4,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    base = buf.data_ptr()
    d_sh, d_p, d_n = base, base + rec, base + rec + tab                             # the free record lies behind the normals
    for out in (d_sh, d_sh + rec - 4, d_p - rec + 4, d_n, d_n + tab - 4, d_p + 4):
        with pytest.raises(abi.MiError) as ei:
            gpu_ctx.lightmap_finish_sh_device(Wd, Hd, d_sh, d_p, d_n, out)
        assert ei.value.code == abi.MI_ERR_INVALID and "overlap" in str(ei.value)
    torch.cuda.synchronize(dev)
    assert (buf.cpu().numpy() == -7.0).all()
    gpu_ctx.lightmap_finish_sh_device(Wd, Hd, d_sh, d_p, d_n, d_n + tab)            # touching is not overlapping
    torch.cuda.synchronize(dev)


def test_a_nan_texel_spoils_its_footprint_only(gpu_ctx):
    name, sh, P, N, _ = BATTERIES[1]
    Hc, Wc = sh.shape[:2]
    covered = N.any(axis=-1)
    ys, xs = np.nonzero(covered)
    k = int(np.argmin(np.maximum(np.abs(ys - Hc // 2), np.abs(xs - Wc // 2))))
    y0, x0 = int(ys[k]), int(xs[k])
    dirty = sh.copy()
    dirty[y0, x0, 4, 1] = np.nan                                                   # one channel of a plane that feeds no weight
    levels, dilate = 3, 4
    params = dict(levels=levels, normal_power_log2=5, sigma_color=6.0, dilate=dilate)
    want, want_valid = finish_reference(name, sh, P, N, params)
    out, valid = gpu_ctx.lightmap_finish_sh(dirty, P, N, **params)
    yy, xx = np.mgrid[0:Hc, 0:Wc]
    far = np.maximum(np.abs(yy - y0), np.abs(xx - x0)) > 2 * (2 ** levels - 1) + dilate
    assert far.sum() > 1000
    assert np.array_equal(valid, want_valid) and np.array_equal(bits(out)[far], bits(want)[far])
    near = ~far
    assert np.isnan(out[near]).any() and np.array_equal(bits(out[:, :, 0, :]), bits(want[:, :, 0, :]))     # and plane 0 never saw it


# ---------------------------------------------------------------- 8. the evaluation
@pytest.mark.parametrize("count", [1, 63, 64, 65, 1000])
def test_eval_has_the_helpers_bits(gpu_ctx, count):
    import torch
    sh, nrm = _records_and_normals(count, 100 + count)
    want = lightmap_sh_eval(sh, nrm)
    got = gpu_ctx.lightmap_sh_eval(sh, nrm)
    assert got.shape == (count, 3) and np.array_equal(bits(got), bits(want))
    assert gpu_ctx.last_kernel_ms() > 0.0
    dev = torch.device("cuda:0")
    t_sh, t_n = torch.from_numpy(sh).to(dev), torch.from_numpy(nrm).to(dev)
    out = torch.full((count + 1, 3), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    gpu_ctx.lightmap_sh_eval_device(count, t_sh.data_ptr(), t_n.data_ptr(), out.data_ptr())
    torch.cuda.synchronize(dev)
    res = out.cpu().numpy()
    assert np.array_equal(bits(res[:count]), bits(want)) and (res[count] == -7.0).all()      # not one lane past n


def test_eval_of_the_cube_bake(gpu_ctx):
    sh, f32, _, _, _, sc, cube = cube_bake(gpu_ctx)
    _, n1, _ = gpu_ctx.lightmap_texels(cube, 32, 32, rows=1, offset=1e-3)
    E = gpu_ctx.lightmap_sh_eval(sh, n1)                                           # an atlas with lightmap_texels' [1, H, W, 3] normals
    assert E.shape == (32, 32, 3) and np.array_equal(bits(E), bits(lightmap_sh_eval(sh, n1[0])))
    covered = n1[0].any(axis=-1)
    assert np.isfinite(E).all() and not bits(E)[~covered].any()
    # every sample of a texel lies in the hemisphere about its face's normal, where the order-2 cosine lobe is positive (its minimum,
    # at the horizon, is 1/4 - 5/32): a channel with a positive mean has a positive E
    lit = covered & (f32.min(axis=-1) > 1e-3)
    up = lit & (n1[0][..., 1] > 0.99)                                               # the face under the ceiling light
    print(f"cube bake: {int(lit.sum())} lit texels, {int(up.sum())} on the top face; E / (pi mean) there {float((E[up] / (np.pi * f32[up])).mean()):.3f}")
    assert lit.sum() > 200 and up.sum() > 50 and (E[lit] > 0).all()


# ---------------------------------------------------------------- 9. refusals
def test_refusals_launch_nothing_and_leave_render_alone(gpu_ctx, orc):
    lib = abi.load()
    big = scenes.config2(96, 64, 4, 6)
    gpu_ctx.upload(big.flatten())
    before = gpu_ctx.render(big.camera, seed=1, want_sig=True)[:3]
    sc = SCENES["config1"][0]()
    gpu_ctx.upload(sc.flatten())
    p, n = (np.array(t) for t in point_table(orc, "config1", "aa"))
    f32 = np.full((H, W, 3), -7.0, np.float32)
    sh = np.full((H, W, 9, 3), -7.0, np.float32)
    h = gpu_ctx._h
    nan = float("nan")
    cube_pod, keep = mesh_pod(fb.cube_mesh())

    def call(ctx=h, rows=4, pts=p.ctypes.data, nrm=n.ctypes.data, out_sh=sh.ctypes.data, variant=0, rank=0, world=1, form="host", **cam_kw):
        cam = SCENES["config1"][0]().camera
        for k, v in cam_kw.items():
            setattr(cam, k, v)
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=SEED, rank=rank, world=world, variant=variant, want_signature=0, flags=0, max_state_bytes=0)
        if form == "device":      # every refusal comes before a pointer is used: the host arrays stand in for device memory here
            rc = lib.mi_render_points_sh_device(ctx, C.byref(pod), C.byref(opts), pts, nrm, rows, 0, cam.aa_sample_count, None, out_sh,
                                                f32.ctypes.data, None, None, None)
        elif form == "bake":
            rc = lib.mi_bake_lightmap_sh(ctx, C.byref(pod), C.byref(opts), C.byref(cube_pod) if pts else None, abi.MI_LM_JITTER if rows == 4 else 0,
                                         1e-3, out_sh, f32.ctypes.data, None, None, None, None)
        else:
            rc = lib.mi_render_points_sh(ctx, C.byref(pod), C.byref(opts), pts, nrm, rows, out_sh, f32.ctypes.data, None, None, None)
        msg = lib.mi_last_error().decode()
        assert rc == abi.MI_OK or len(msg) > 10, (rc, msg)
        return rc, msg

    assert call()[0] == abi.MI_OK and f32.max() > 0 and np.abs(sh).max() > 0 and not (sh == -7.0).any()
    f32[:] = -7.0
    sh[:] = -7.0
    ms_before, counts_before = gpu_ctx.last_kernel_ms(), gpu_ctx.last_pipeline_counts()
    for form in ("host", "device", "bake"):
        kw = dict(form=form)
        assert call(path_samples=2, **kw)[0] == abi.MI_ERR_UNSUPPORTED
        assert call(shading_mode=ShadingMode.Phong, **kw)[0] == abi.MI_ERR_UNSUPPORTED
        for variant in (abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_RECURSIVE, 99):
            assert call(variant=variant, **kw)[0] == abi.MI_ERR_UNSUPPORTED, variant
        for bad in (dict(path_samples=0), dict(max_trace_dist=nan), dict(gamma=0.0), dict(screen_width=0), dict(screen_width=40000),
                    dict(aa_sample_count=0)):
            assert call(**bad, **kw)[0] == abi.MI_ERR_INVALID, bad
        if form != "bake":
            for rows in (0, 2, 3, 5, 16):
                assert call(rows=rows, **kw)[0] == abi.MI_ERR_INVALID, rows
            assert call(nrm=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(pts=None, **kw)[0] == abi.MI_ERR_INVALID                        # bake: the mesh
        assert call(ctx=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(rank=1, world=1, **kw)[0] == abi.MI_ERR_INVALID
    for form in ("host", "bake"):
        assert call(rank=0, world=2, form=form)[0] == abi.MI_ERR_INVALID            # the host forms render a whole image
        rc, msg = call(out_sh=None, form=form)                                      # and require out_sh
        assert rc == abi.MI_ERR_INVALID and "out_sh" in msg
    fresh = Context(0)
    try:
        for form in ("host", "device", "bake"):
            assert call(ctx=fresh._h, form=form)[0] == abi.MI_ERR_NO_SCENE
    finally:
        fresh.close()
    # the finish and the evaluation
    _, img, P, N, _ = fb.ragged_battery(31, 33)
    rec = sh_records(img)
    Hf, Wf = img.shape[:2]
    out = np.full((Hf, Wf, 9, 3), -7.0, np.float32)
    valid = np.full((Hf, Wf), 9, np.uint8)

    def finish(ctx=h, w=Wf, hh=Hf, image=rec.ctypes.data, points=P.ctypes.data, normals=N.ctypes.data, levels=3, npow=5, sigma_plane=INF,
               reach=INF, sigma_color=INF, dilate=4, out_sh=out.ctypes.data, device=False):
        if device:
            rc = lib.mi_lightmap_finish_sh_device(ctx, w, hh, image, points, normals, levels, npow, sigma_plane, reach, sigma_color, dilate,
                                                  out_sh, valid.ctypes.data, None)
        else:
            rc = lib.mi_lightmap_finish_sh(ctx, w, hh, image, points, normals, levels, npow, sigma_plane, reach, sigma_color, dilate, out_sh,
                                           valid.ctypes.data)
        assert rc == abi.MI_OK or len(lib.mi_last_error().decode()) > 10
        return rc

    for kw in [dict(image=None), dict(points=None), dict(normals=None), dict(out_sh=None), dict(ctx=None), dict(w=0), dict(hh=0), dict(w=32769),
               dict(hh=32769), dict(levels=9), dict(npow=8), dict(dilate=257), dict(sigma_plane=nan), dict(sigma_plane=0.0), dict(reach=nan),
               dict(reach=-INF), dict(sigma_color=nan), dict(sigma_color=0.0), dict(sigma_color=-0.5)]:
        for device in (False, True):
            assert finish(device=device, **kw) == abi.MI_ERR_INVALID, (kw, device)
    E = np.full((Hf * Wf, 3), -7.0, np.float32)
    for device in (False, True):
        tail = (None,) if device else ()
        fn = lib.mi_lightmap_sh_eval_device if device else lib.mi_lightmap_sh_eval
        for args in ((h, Hf * Wf, None, N.ctypes.data, E.ctypes.data), (h, Hf * Wf, rec.ctypes.data, None, E.ctypes.data),
                     (h, Hf * Wf, rec.ctypes.data, N.ctypes.data, None), (None, Hf * Wf, rec.ctypes.data, N.ctypes.data, E.ctypes.data)):
            assert fn(*args, *tail) == abi.MI_ERR_INVALID and len(lib.mi_last_error().decode()) > 10
        assert fn(h, 0, rec.ctypes.data, N.ctypes.data, E.ctypes.data, *tail) == abi.MI_OK                  # no point: MI_OK, nothing launched
    assert np.all(f32 == -7.0) and np.all(sh == -7.0) and (out == -7.0).all() and (valid == 9).all() and (E == -7.0).all()
    assert gpu_ctx.last_kernel_ms() == ms_before and gpu_ctx.last_pipeline_counts() == counts_before      # nothing was launched
    assert finish(levels=8, npow=7, dilate=256) == abi.MI_OK and (out != -7.0).all()                      # the limits themselves are legal
    with pytest.raises(ValueError):                                                 # the Python mirror checks before any call
        gpu_ctx.render_points_sh(sc.camera, p[:2], n[:2])
    del keep
    # and an ordinary render afterwards is what it was
    gpu_ctx.upload(big.flatten())
    assert same(gpu_ctx.render(big.camera, seed=1, want_sig=True)[:3], before)
    assert gpu_ctx.last_reduce_psh_ms() == 0.0
