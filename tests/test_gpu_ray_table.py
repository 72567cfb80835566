"""Ray-table rendering (mi_render_rays / mi_render_rays_device): caller-made rays through the wavefront pipeline, against the oracle.

The oracle side of every comparison is orc_shade per (pixel, sample) on the stream (seed, y*W + x, s), summed in f32 in sample order
and divided by n in f32 (tracing.rs:238-241), then orc_tonemap_pixel for the bytes.  Bars: those of tests/test_gpu_parity.py::compare
— per-channel RMS <= 1e-3, max |diff| <= 2e-5 * max(1, |ref|), u8 within 1 LSB.  Images are 75 x 41: ragged in both tile directions,
so every render has padded lanes (which must not read the table)."""
import ctypes as C

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Context, ConvexVolume, Isotropic, Lambertian, Plane, Sphere, StaticMesh, Triangle, abi, cgmath,
                                     dist as pdist, scenes)
from cs397raytracingsp22_amd.tracing import ShadingMode, equirect_ray_table

from test_gpu_parity import RMS_TOL
from test_gpu_ray_queries import long_triangle_list
from test_gpu_volume_boundaries import cube_volume_scene

pytestmark = pytest.mark.gpu

W, H = 75, 41
SEED = 5


def _sized(sc, aa, depth):
    cam = sc.camera
    cam.screen_width, cam.screen_height, cam.aa_sample_count, cam.path_depth = W, H, aa, depth
    return sc


def rare_top_scene():
    """The top-level tree beside the rare kinds: long_triangle_list() + a sphere-bounded ConvexVolume + a Plane (no general boundary)."""
    sc = long_triangle_list()
    sc.objects += [ConvexVolume(Sphere((0.6, 1.6, 0.9), 0.9, Lambertian(albedo=(0.6, 0.6, 0.6))), Isotropic(albedo=(0.9, 0.8, 0.7)), 1.5),
                   Plane((0.0, -0.5, 0.0), (0.0, 1.0, 0.0), Lambertian(albedo=(0.4, 0.5, 0.4), emission=(0.05, 0.05, 0.05)))]
    return sc


def gv_top_scene():
    """The top-level tree beside a general boundary: cube_volume_scene() + the 120 small Triangles of long_triangle_list()."""
    sc = cube_volume_scene()
    sc.objects += long_triangle_list().objects[-120:]
    return sc


def gv_mesh_top_scene():
    """gv_top + a small untextured teapot near the opening of the box: the later passes take the M = 1 state form beside the tree and the
    general volume, and the scene's mesh trees are staged in LDS beside the tree's pools."""
    sc = gv_top_scene()
    xf = cgmath.mul(cgmath.from_translation(TEAPOT_AT), cgmath.from_angle_x(-90.0), cgmath.from_scale(TEAPOT_SCALE))
    sc.objects.append(StaticMesh(scenes.load_asset_mesh("teapot"), Lambertian(albedo=(0.6, 0.3, 0.2), emission=(0.2, 0.2, 0.2)), [None] * 5, xf))
    return sc


TEAPOT_AT, TEAPOT_SCALE = (1.45, 0.62, 1.8), 1.7

# scene -> (builder, aa_sample_count, an eye inside the scene for the panorama); between them they select every RAYS form of wf_main
SCENES = {
    "config1": (lambda: _sized(scenes.config1(), 4, 8), (0.3, 2.5, 1.0)),                      # plain
    "config2": (lambda: _sized(scenes.config2(), 4, 8), (0.3, 3.5, 1.5)),                      # teapot: LDS walker, class B
    "config5": (lambda: _sized(scenes.config5(), 4, 8), (0.5, 3.5, 2.0)),                      # RARE: volume + glass
    "cube_volume": (lambda: _sized(cube_volume_scene(), 4, 8), (-0.5, 4.0, 2.0)),              # GV: a mesh-bounded ConvexVolume
    "long_list": (lambda: _sized(long_triangle_list(), 4, 6), (0.2, 5.5, 2.5)),                # TOP: >= 96 small triangles in a tree
    "config4": (lambda: _sized(scenes.config4(tex_size=64), 4, 8), (1.5, 1.0, 2.0)),           # textured class B
    "head": (lambda: _sized(scenes.head_scene(), 3, 8), (0.0, 2.0, 4.0)),                      # two-stage meshes; aa = 3 is no square
    "rare_top": (lambda: _sized(rare_top_scene(), 4, 6), (0.2, 5.5, 2.5)),                     # RARE + TOP: a Plane and a sphere volume behind the tree
    "gv_top": (lambda: _sized(gv_top_scene(), 4, 6), (-0.5, 4.0, 2.0)),                        # GV + TOP
    "gv_mesh_top": (lambda: _sized(gv_mesh_top_scene(), 4, 6), (-0.5, 4.0, 2.0)),              # GV + TOP with a mesh: M = 1 state passes
}


def fan_table(cam, rows, seed):
    """A seeded pinhole fan from the scene camera's eye towards the scene: direction ((x + jx - W/2) / H, (H/2 - y - jy) / H, -0.6),
    NOT normalised, jitter in [0, 1)^2 per (row, pixel)."""
    j = np.random.default_rng(seed).random((2, rows, H, W))
    x = (np.arange(W)[None, None, :] + j[0] - 0.5 * W) / H
    y = (0.5 * H - np.arange(H)[None, :, None] - j[1]) / H
    d = np.ascontiguousarray(np.stack([x, y, np.full_like(x, -0.6)], axis=-1), dtype=np.float32)
    o = np.ascontiguousarray(np.broadcast_to(np.asarray(cam.eyepoint, np.float32), d.shape))
    return o, d


def make_table(name, kind, rows, seed=21):
    sc = SCENES[name][0]()
    rows = sc.camera.aa_sample_count if rows == "aa" else 1
    if kind == "fan":
        return fan_table(sc.camera, rows, seed)
    return equirect_ray_table(W, H, SCENES[name][1], samples=rows, seed=seed)


def oracle_image(orc, flat, cam, o, d, seed):
    """(f32 mean [H, W, 3], u8 [H, W, 3]) the reference's way: orc_shade per (pixel, sample), f32 sum in sample order, / n in f32."""
    lib = orc.load()
    osc = orc.OracleScene(flat)
    pod = cam.to_pod()
    S, rows = cam.aa_sample_count, o.shape[0]
    fp = C.POINTER(C.c_float)
    samples = np.zeros((S, H, W, 3), np.float32)
    ob, db, sb = o.ctypes.data, d.ctypes.data, samples.ctypes.data
    for s in range(S):
        row = s if rows > 1 else 0
        for p in range(H * W):
            off = (row * H * W + p) * 12
            rc = lib.orc_shade(osc._h, C.byref(pod), C.cast(ob + off, fp), C.cast(db + off, fp), seed, p, s,
                               C.cast(sb + (s * H * W + p) * 12, fp))
            assert rc == 0
    osc.close()
    acc = np.zeros((H, W, 3), np.float32)
    for s in range(S):
        acc = acc + samples[s]                              # final_color += shade_ray(..)  tracing.rs:238
    mean = acc / np.float32(S)                              # :241
    u8 = np.stack([orc.tonemap_pixel(px, cam.gamma) for px in mean.reshape(-1, 3)]).reshape(H, W, 3)
    return mean, u8


def assert_within_bars(f32, u8, r32, r8, what):
    assert np.isfinite(r32).all(), what
    err = np.abs(f32.astype(np.float64) - r32.astype(np.float64))
    rms = [float(np.sqrt(np.mean(err[..., ch] ** 2))) for ch in range(3)]
    rel = float((err / np.maximum(1.0, np.abs(r32.astype(np.float64)))).max())
    print(f"{what}: rms {rms}, max relative diff {rel:.3e}, lit pixels {int((r32.sum(axis=-1) > 0).sum())}")
    assert max(rms) <= RMS_TOL, (what, rms)
    assert rel <= 2e-5, (what, rel)
    if u8 is not None:
        assert int(np.abs(u8.astype(int) - r8.astype(int)).max()) <= 1, what


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    return all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


# ---------------------------------------------------------------- 1. against the oracle
CASES = [(n, k, r) for n in SCENES for k, r in (("fan", "aa"), ("equirect", 1))] + \
        [("config2", "fan", 1), ("config2", "equirect", "aa"), ("config5", "fan", 1), ("config5", "equirect", "aa")]


@pytest.mark.parametrize("name,kind,rows", CASES)
def test_against_the_oracle(gpu_ctx, orc, name, kind, rows):
    sc = SCENES[name][0]()
    if name == "long_list":
        assert sum(isinstance(ob, Triangle) for ob in sc.objects) >= 105
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    o, d = make_table(name, kind, rows)
    assert o.shape[0] == (1 if rows == 1 else sc.camera.aa_sample_count)
    f32, u8, sig, st = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_sig=True)
    assert st.samples == W * H * sc.camera.aa_sample_count
    assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    g32, g8, none, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_sig=False)
    assert none is None and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    assert np.array_equal(bits(f32), bits(g32)) and np.array_equal(u8, g8)          # signatures on / off: the same image, bit for bit
    r32, r8 = oracle_image(orc, flat, sc.camera, o, d, SEED)
    assert int((r32.sum(axis=-1) > 0).sum()) >= 100                                 # the reference is not vacuous (the open HEAD scene is the darkest)
    assert_within_bars(f32, u8, r32, r8, f"{name} {kind} rows={rows}")


# ---------------------------------------------------------------- 2. against the existing query
@pytest.mark.parametrize("name", ["config2", "config5", "head"])
def test_one_sample_agrees_with_shade_rays(gpu_ctx, name):
    """aa_sample_count = 1: sample 0 of pixel (x, y) is mi_shade_rays' ray y*W + x with first_key = 0 — the keying is (seed, y*W+x, s)."""
    sc = SCENES[name][0]()
    sc.camera.aa_sample_count = 1
    gpu_ctx.upload(sc.flatten())
    o, d = fan_table(sc.camera, 1, 3)
    f32, _, _, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_u8=False)
    ref = gpu_ctx.shade_rays(sc.camera, o.reshape(-1, 3), d.reshape(-1, 3), seed=SEED, first_key=0).reshape(H, W, 3)
    assert int((ref.sum(axis=-1) > 0).sum()) >= 50
    assert_within_bars(f32, None, ref, None, f"{name} vs shade_rays")
    other = gpu_ctx.shade_rays(sc.camera, o.reshape(-1, 3), d.reshape(-1, 3), seed=SEED, first_key=1).reshape(H, W, 3)
    assert not np.array_equal(other, ref)                                           # and the key matters in this scene


# ---------------------------------------------------------------- 3. exactness across schedules
def device_render(ctx, cam, o, d, world, seed, flags=0, split=None, max_state_bytes=0):
    """The device form: every rank's tiles in turn into a gathered buffer, K3 + K4 on the device, signatures un-permuted with the
    numpy mirror of K3's mapping.  split = k renders [0, k) and [k, aa) as two progressive calls with the accumulator copied out to
    the host and back in between."""
    import torch
    dev = torch.device("cuda:0")
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    padded = pdist.tiles_padded(W, H, world)
    gathered = torch.full((world, padded, pdist.TILE_PIXELS, 3), float("nan"), dtype=torch.float32, device=dev)
    gsig = torch.zeros((world, padded, pdist.TILE_PIXELS), dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    samples = 0
    for r in range(world):
        kw = dict(seed=seed, rank=r, world=world, flags=flags, max_state_bytes=max_state_bytes)
        if split is None:
            st = ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), o.shape[0], gathered[r].data_ptr(), gsig[r].data_ptr(), **kw)
            samples += st.samples
        else:
            acc = torch.full((padded * pdist.TILE_PIXELS, 4), float("nan"), dtype=torch.float32, device=dev)
            # (signatures are wanted in EVERY slice, as ProgressiveRender asks: a slice traced without them adds nothing to their sums)
            st = ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), o.shape[0], None, gsig[r].data_ptr(), 0, split, acc.data_ptr(), **kw)
            samples += st.samples
            saved = acc.cpu()
            acc2 = saved.to(dev)                           # "another process": the sums travel through the host
            torch.cuda.synchronize(dev)
            st = ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), o.shape[0], gathered[r].data_ptr(), gsig[r].data_ptr(),
                                        split, cam.aa_sample_count, acc2.data_ptr(), **kw)
            samples += st.samples
    image = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    ctx.unpermute_device(cam, world, gathered.data_ptr(), image.data_ptr())
    ctx.tonemap_device(cam, image.data_ptr(), u8.data_ptr())
    torch.cuda.synchronize(dev)
    assert not torch.isnan(gathered).any()                 # padding slots and pixels outside the image are written as zeros
    r_of, idx = pdist.compact_index(W, H, world)
    sig = gsig.cpu().numpy().view(np.uint32).reshape(world, -1)[r_of, idx]
    assert samples == W * H * cam.aa_sample_count
    return image.cpu().numpy(), u8.cpu().numpy(), sig


@pytest.mark.parametrize("name", ["config2", "long_list", "head", "rare_top", "gv_mesh_top"])
def test_schedules_are_bit_identical(gpu_ctx, name):
    sc = SCENES[name][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    o, d = make_table(name, "fan", "aa")
    base = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True)[:3]
    assert base[0].max() > 0 and len(np.unique(base[2])) > 100
    launches = gpu_ctx.last_pipeline_ms()["launches"]
    # one sample per batch: the budget of one sample of every padded pixel (208 B per path, 72 B more with a two-stage mesh)
    npix = pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS
    got = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True, max_state_bytes=npix * (2 * 6 * 16 + 16 + 72))[:3]
    assert gpu_ctx.last_pipeline_ms()["launches"] > launches
    assert same(got, base), "one sample per batch"
    for flags in (abi.MI_OPT_NO_LIST_TREE, abi.MI_OPT_REFERENCE_WALK, abi.MI_OPT_TWO_STAGE, abi.MI_OPT_NO_TILE_MASKS):
        got = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True, flags=flags)[:3]
        assert same(got, base), f"flags {flags}"
        assert gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0
    for world in (1, 2, 3):
        assert same(device_render(gpu_ctx, cam, o, d, world, SEED), base), f"world {world}"
    for k in (1, cam.aa_sample_count - 1):
        assert same(device_render(gpu_ctx, cam, o, d, 1, SEED, split=k), base), f"progressive split at {k}"
    assert same(device_render(gpu_ctx, cam, o, d, 2, SEED, split=2), base), "progressive, two ranks"


# ---------------------------------------------------------------- 4. edges
def test_path_depth_zero_is_black(gpu_ctx):
    sc = SCENES["config2"][0]()
    sc.camera.path_depth = 0
    gpu_ctx.upload(sc.flatten())
    o, d = fan_table(sc.camera, 1, 1)
    f32, u8, sig, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_sig=True)
    assert not f32.any() and not u8.any() and not np.signbit(f32).any()
    g32, _, _, _ = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED)
    assert not g32.any()


def test_one_pixel_image(gpu_ctx, orc):
    sc = scenes.config5(1, 1, 4, 8)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    o = np.tile(np.asarray(sc.camera.eyepoint, np.float32), (4, 1, 1, 1))
    d = np.array([[0.0, -0.1, -1.0], [0.02, -0.3, -1.0], [-0.3, -0.2, -1.0], [0.1, 0.4, -1.0]], np.float32).reshape(4, 1, 1, 3)
    f32, u8, _, st = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED)
    assert st.samples == 4 and f32.shape == (1, 1, 3)
    osc = orc.OracleScene(flat)
    acc = np.zeros(3, np.float32)
    for s in range(4):
        acc = acc + osc.shade(sc.camera, o[s, 0, 0], d[s, 0, 0], seed=SEED, pixel=0, sample=s)
    osc.close()
    ref = acc / np.float32(4)
    assert ref.sum() > 0
    assert float((np.abs(f32[0, 0].astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))).max()) <= 2e-5
    assert int(np.abs(u8[0, 0].astype(int) - orc.tonemap_pixel(ref, sc.camera.gamma).astype(int)).max()) <= 1


@pytest.mark.parametrize("name", ["config1", "config2", "head"])
def test_bad_rays_among_finite_ones_leave_the_finite_pixels_alone(gpu_ctx, name):
    """Non-finite and zero-length directions, non-finite origins: MI_OK, and every pixel whose rays are finite has exactly the value it
    has in a table without the bad rays (a pixel's samples depend on nothing but its own rays and its own stream)."""
    sc = SCENES[name][0]()
    cam = sc.camera
    gpu_ctx.upload(sc.flatten())
    o, d = fan_table(cam, cam.aa_sample_count, 8)
    good = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True)[:3]
    nan, inf = np.float32("nan"), np.float32("inf")
    bad_d = [(nan, nan, nan), (0.0, 0.0, 0.0), (inf, 0.0, -1.0), (0.0, -inf, 0.0), (nan, 0.1, -1.0), (0.0, 0.0, nan), (-inf, inf, -inf),
             (1e38, 1e38, -1e38), (1e-45, 0.0, 0.0)]
    bad_o = [(nan, 0.0, 0.0), (inf, inf, inf), (0.0, -inf, 5.0), (3e38, 3.0, 6.6)]
    rng = np.random.default_rng(2)
    mask = np.zeros((H, W), bool)
    o2, d2 = o.copy(), d.copy()
    pix = rng.choice(H * W, 400, replace=False)
    for k, p in enumerate(pix):
        y, x = divmod(int(p), W)
        s = k % cam.aa_sample_count if k % 3 else slice(None)                     # one sample of the pixel, or all of them
        if k % 4 == 3:
            o2[s, y, x] = bad_o[k % len(bad_o)]
        else:
            d2[s, y, x] = bad_d[k % len(bad_d)]
        mask[y, x] = True
    mask[[0, H - 1, 0, H - 1], [0, 0, W - 1, W - 1]] = True                       # the image corners, next to the padded lanes
    for y, x in ((0, 0), (H - 1, 0), (0, W - 1), (H - 1, W - 1)):
        d2[:, y, x] = (nan, nan, nan)
    got = gpu_ctx.render_rays(cam, o2, d2, seed=SEED, want_sig=True)[:3]           # MI_OK, or check() raises
    keep = ~mask
    assert keep.sum() > 2000
    for a, b in zip(got, good):
        assert np.array_equal(bits(a)[keep], bits(b)[keep])
    again = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True)[:3]           # and the context is as good as before
    assert same(again, good)


def test_ignored_camera_fields_and_a_sample_count_that_is_no_square(gpu_ctx):
    sc = SCENES["config5"][0]()
    cam = sc.camera
    cam.aa_sample_count = 3
    gpu_ctx.upload(sc.flatten())
    o, d = fan_table(cam, 3, 4)
    want = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True)[:3]
    nan, inf = float("nan"), float("inf")
    cam.eyepoint, cam.view_dir, cam.up = (nan, inf, -inf), (0.0, 0.0, 0.0), (nan, nan, nan)
    cam.projection_mode, cam.focal_length, cam.focus_dist, cam.lens_radius = 77, nan, -inf, nan
    got = gpu_ctx.render_rays(cam, o, d, seed=SEED, want_sig=True)[:3]
    assert got[0].max() > 0 and same(got, want)
    with pytest.raises(abi.MiError):                                               # mi_render itself still refuses this camera
        gpu_ctx.render(cam)


def test_refusals_launch_nothing(gpu_ctx):
    lib = abi.load()
    sc = SCENES["config1"][0]()
    gpu_ctx.upload(sc.flatten())
    o, d = fan_table(sc.camera, 4, 1)
    f32 = np.full((H, W, 3), -7.0, np.float32)
    h, po, pd, pf = gpu_ctx._h, o.ctypes.data, d.ctypes.data, f32.ctypes.data
    nan = float("nan")

    def call(ctx=h, rows=4, orig=po, dirs=pd, variant=0, rank=0, world=1, device=False, **cam_kw):
        cam = SCENES["config1"][0]().camera
        for k, v in cam_kw.items():
            setattr(cam, k, v)
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=SEED, rank=rank, world=world, variant=variant, want_signature=0, flags=0, max_state_bytes=0)
        if device:        # every refusal comes before a pointer is used: the host arrays stand in for device memory here
            rc = lib.mi_render_rays_device(ctx, C.byref(pod), C.byref(opts), orig, dirs, rows, 0, cam.aa_sample_count, None, pf, None, None, None)
        else:
            rc = lib.mi_render_rays(ctx, C.byref(pod), C.byref(opts), orig, dirs, rows, pf, None, None, None)
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
        assert rc == abi.MI_ERR_UNSUPPORTED and "mi_shade_rays" in msg
        for variant in (abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_VOTED_DIAG, abi.MI_VARIANT_RECURSIVE, 2, 99):
            assert call(variant=variant, **kw)[0] == abi.MI_ERR_UNSUPPORTED, variant
        assert call(variant=abi.MI_VARIANT_WAVEFRONT, rows=3, **kw)[0] == abi.MI_ERR_INVALID      # (a legal variant, a bad row count)
        for bad in (dict(path_samples=0), dict(max_trace_dist=nan), dict(gamma=0.0), dict(gamma=nan), dict(gamma=float("inf")),
                    dict(screen_width=0), dict(screen_height=0), dict(screen_width=40000), dict(aa_sample_count=0), dict(shading_mode=9)):
            assert call(**bad, **kw)[0] == abi.MI_ERR_INVALID, bad
        for rows in (0, 2, 3, 5, 16):
            assert call(rows=rows, **kw)[0] == abi.MI_ERR_INVALID, rows
        assert call(orig=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(dirs=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(ctx=None, **kw)[0] == abi.MI_ERR_INVALID
        assert call(rank=1, world=1, **kw)[0] == abi.MI_ERR_INVALID
    assert call(rank=0, world=2)[0] == abi.MI_ERR_INVALID                           # the host form renders a whole image
    assert np.all(f32 == -7.0)                                                      # nothing was written ...
    assert gpu_ctx.last_kernel_ms() == ms_before and gpu_ctx.last_pipeline_counts() == counts_before      # ... and nothing was launched
    fresh = Context(0)
    try:
        for device in (False, True):
            rc, msg = call(ctx=fresh._h, device=device)
            assert rc == abi.MI_ERR_NO_SCENE
    finally:
        fresh.close()
    assert call()[0] == abi.MI_OK and f32.max() > 0                                 # the context is still good
    # the progressive rules of mi_render_samples_device hold for a table too
    import torch
    cam = sc.camera
    t_o, t_d = torch.from_numpy(o).to("cuda:0"), torch.from_numpy(d).to("cuda:0")
    acc = torch.zeros((pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS, 4), dtype=torch.float32, device="cuda:0")
    out = torch.zeros((pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS, 3), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    for b, e, a, c in ((2, 2, acc, out), (3, 2, acc, out), (0, 5, acc, out), (0, 2, None, None), (0, 4, acc, None), (0, 4, None, None)):
        with pytest.raises(abi.MiError) as ei:
            gpu_ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), 4, c.data_ptr() if c is not None else None, None, b, e,
                                       a.data_ptr() if a is not None else None)
        assert ei.value.code == abi.MI_ERR_INVALID, (b, e)


def test_render_is_bit_identical_before_and_after_a_ray_table_render(gpu_ctx):
    sc = scenes.config2(240, 136, 16, 10)
    gpu_ctx.upload(sc.flatten())
    a32, a8, asig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    gpu_ctx.render(sc.camera, seed=1)
    dead = gpu_ctx.last_pipeline_counts()["dead_tile_samples"]
    assert dead > 0                                                                 # the camera render culls dead tiles ...
    small = SCENES["config2"][0]().camera
    o, d = fan_table(small, 1, 6)
    t32, _, _, _ = gpu_ctx.render_rays(small, o, d, seed=1)
    assert t32.max() > 0 and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == 0      # ... the table render does not
    b32, b8, bsig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    assert np.array_equal(bits(a32), bits(b32)) and np.array_equal(asig, bsig) and np.array_equal(a8, b8)
    c32, _, _, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=False)
    assert np.array_equal(bits(a32), bits(c32)) and gpu_ctx.last_pipeline_counts()["dead_tile_samples"] == dead


# ---------------------------------------------------------------- 5. entry points
@pytest.mark.parametrize("name,rows", [("config4", "aa"), ("config5", 1)])
def test_host_and_device_forms_give_the_same_bytes(gpu_ctx, name, rows):
    sc = SCENES[name][0]()
    gpu_ctx.upload(sc.flatten())
    o, d = make_table(name, "equirect", rows)
    host = gpu_ctx.render_rays(sc.camera, o, d, seed=SEED, want_sig=True)[:3]
    assert host[0].max() > 0
    assert same(device_render(gpu_ctx, sc.camera, o, d, 1, SEED), host)
