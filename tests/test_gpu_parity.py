"""GPU parity: the HIP path (through the C ABI) against the CPU oracle on the same seeded
inputs.  Bars:
  * path signatures (per-pixel hash of every hit distance, hit object and the final RNG
    state of every sample) must be BIT-IDENTICAL: every path made the same decisions.
  * linear f32 radiance: per-channel RMS <= 1e-3 (north_star) — in practice ~1e-7, because
    the GPU accumulates T*E forward while the reference nests the products (tracing.rs:316,321);
    the test also enforces max |diff| <= 2e-5 * max(1, |ref|).
  * u8 image: <= 1 LSB (powf of the two libms may differ in the last bit).
"""
import numpy as np
import pytest

from cs397raytracingsp22_amd import abi, scenes

pytestmark = pytest.mark.gpu

RMS_TOL = 1e-3          # BASELINE.json north_star: <= 1e-3 per-channel RMS vs CPU reference


def compare(ctx, orc, sc, seed=1, variant=abi.MI_VARIANT_DEFAULT, window=None):
    flat = sc.flatten()
    ctx.upload(flat)
    f32, u8, sig, st = ctx.render(sc.camera, seed=seed, want_sig=True, variant=variant)
    o = orc.OracleScene(flat)
    r32, r8, rsig, _ = o.render(sc.camera, seed=seed, window=window)
    if window is not None:
        x0, y0, w, h = window
        f32, u8, sig = f32[y0:y0 + h, x0:x0 + w], u8[y0:y0 + h, x0:x0 + w], sig[y0:y0 + h, x0:x0 + w]
    bad = int((sig != rsig).sum())
    assert bad == 0, f"{bad}/{sig.size} pixels took a different path than the oracle"
    for ch in range(3):
        rms = float(np.sqrt(np.mean((f32[..., ch].astype(np.float64) - r32[..., ch]) ** 2)))
        assert rms <= RMS_TOL, (ch, rms)
    err = np.abs(f32.astype(np.float64) - r32)
    assert float((err / np.maximum(1.0, np.abs(r32))).max()) <= 2e-5
    assert int(np.abs(u8.astype(int) - r8.astype(int)).max()) <= 1
    assert float((u8 != r8).mean()) <= 1e-3
    return st


@pytest.mark.parametrize("variant", [abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_WAVEFRONT])
def test_config1_cornell(gpu_ctx, orc, variant):
    compare(gpu_ctx, orc, scenes.config1(128, 128, 16, 8), variant=variant)


def config2_teapot_scene():
    return scenes.config2(160, 96, 16, 10)


@pytest.mark.parametrize("variant", [abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_WAVEFRONT])
def test_config2_teapot(gpu_ctx, orc, variant):
    compare(gpu_ctx, orc, config2_teapot_scene(), variant=variant)


def test_config2_ragged_edges_and_seed(gpu_ctx, orc):
    # width/height not multiples of the 32-px tile, non-default seed
    compare(gpu_ctx, orc, scenes.config2(75, 41, 9, 6), seed=12345)


def test_defocus(gpu_ctx, orc):
    compare(gpu_ctx, orc, scenes.config2(96, 64, 16, 10, lens_radius=0.05))


def test_work_counters_equal_the_oracle(gpu_ctx, orc):
    """Structural parity: the diagnostic build walks exactly the reference's
    work — same number of path segments, of AABB slab tests and of triangle tests as the oracle
    counts on the reference BVH topology."""
    sc = scenes.config2(96, 64, 16, 10)
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    gpu_ctx.render(sc.camera, seed=5, want_u8=False, variant=abi.MI_VARIANT_VOTED_DIAG)
    d = gpu_ctx.last_diag()
    _, _, _, cnt = orc.OracleScene(flat).render(sc.camera, seed=5, want_u8=False, want_sig=False, want_counters=True)
    assert d["segments"] == cnt["segments"]
    assert d["leaf_lanes"] == cnt["tri_tests"]
    # the oracle counts the root box test of every mesh call; the kernel does it in the A phase
    assert d["slab_tests"] + cnt["mesh_tests"] == cnt["box_tests"]


@pytest.mark.parametrize("name", ["config2", "config5", "head"])
def test_wavefront_segment_counter_equals_the_oracle(gpu_ctx, orc, name):
    """mi_last_pipeline_counts[6], the device-side count of Scene::intersect_ray evaluations bench.py's Msegments/s comes from:
    equal to the oracle's segment count when every sample is traced (signatures on, or the tile masks off), and smaller by
    exactly the dead tiles' samples (one segment each in the oracle: the camera ray that hits nothing) when they are skipped.
    Through the split / fused / tail schedules of the pipeline: the count is per path, not per launch."""
    sc = {"config2": lambda: scenes.config2(160, 90, 16, 10), "config5": lambda: scenes.config5(96, 64, 16, 12),
          "head": lambda: scenes.head_scene(64, 48, 4, 10)}[name]()
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    _, _, _, cnt = orc.OracleScene(flat).render(sc.camera, seed=9, want_u8=False, want_sig=False, want_counters=True)
    gpu_ctx.render(sc.camera, seed=9, want_u8=False, flags=abi.MI_OPT_NO_TILE_MASKS)
    c = gpu_ctx.last_pipeline_counts()
    assert c["segments"] == cnt["segments"] and c["dead_tile_samples"] == 0
    gpu_ctx.render(sc.camera, seed=9, want_u8=False, want_sig=True)
    assert gpu_ctx.last_pipeline_counts()["segments"] == cnt["segments"]
    gpu_ctx.render(sc.camera, seed=9, want_u8=False)                      # dead tiles skipped
    c = gpu_ctx.last_pipeline_counts()
    assert c["segments"] + c["dead_tile_samples"] == cnt["segments"]
    if name == "config2":
        assert c["dead_tile_samples"] > 0                                 # the box is a square in a 16:9 frame
    # several batches: the count is the frame's, not the last batch's
    gpu_ctx.render(sc.camera, seed=9, want_u8=False, max_state_bytes=(2 * 6 * 16 + 16 + 72) * 1024 * 40 * 5)
    c2 = gpu_ctx.last_pipeline_counts()
    assert c2["segments"] + c2["dead_tile_samples"] == cnt["segments"]


# ---- the rest of the Camera / Scene surface: orthographic projection, Phong shading ----
def _mode(sc, **kw):
    for k, v in kw.items():
        setattr(sc.camera, k, v)
    return sc


@pytest.mark.parametrize("variant", [abi.MI_VARIANT_SIMPLE, abi.MI_VARIANT_VOTED, abi.MI_VARIANT_WAVEFRONT])
def test_orthographic_projection(gpu_ctx, orc, variant):
    """tracing.rs:196,200: shared generate_ray, so every kernel variant must agree with the oracle."""
    compare(gpu_ctx, orc, _mode(scenes.config2(96, 64, 16, 10), projection_mode=abi.MI_PROJ_ORTHOGRAPHIC), variant=variant)


def test_orthographic_tilted_camera(gpu_ctx, orc):
    sc = _mode(scenes.config1(64, 64, 16, 8), projection_mode=abi.MI_PROJ_ORTHOGRAPHIC,
               view_dir=(0.0, -0.6, -0.8), up=(0.0, 1.0, 0.0))
    compare(gpu_ctx, orc, sc)


@pytest.mark.parametrize("name", ["config1", "config2", "config4", "config5", "head"])
def test_phong_shading(gpu_ctx, orc, name):
    """Scene::phong_shade_ray (tracing.rs:277-297): primary hit, shadow ray, scatter() for the attenuation —
    spheres, triangles, the teapot BVH, textured ParameterizedMaterial lobes, a ConvexVolume that draws
    random numbers inside both intersect_ray calls."""
    sc = {"config1": lambda: scenes.config1(96, 96, 16, 8), "config2": lambda: scenes.config2(128, 96, 16, 10),
          "config4": lambda: scenes.config4(96, 64, 4, 10, tex_size=64), "config5": lambda: scenes.config5(96, 64, 16, 50),
          "head": lambda: scenes.head_scene(64, 64, 4, 10)}[name]()
    sc.point_light_pos = (0.5, 4.0, 2.5)
    sc.ambient = (0.05, 0.1, 0.15)
    st = compare(gpu_ctx, orc, _mode(sc, shading_mode=abi.MI_SHADE_PHONG))
    assert st.samples == sc.camera.screen_width * sc.camera.screen_height * sc.camera.aa_sample_count


def test_phong_orthographic_ignores_variant(gpu_ctx, orc):
    sc = _mode(scenes.config2(75, 41, 9, 6), shading_mode=abi.MI_SHADE_PHONG, projection_mode=abi.MI_PROJ_ORTHOGRAPHIC)
    compare(gpu_ctx, orc, sc, seed=77, variant=abi.MI_VARIANT_VOTED)


# ---- Scene::shade_ray as written: path_samples scattered rays per hit (tracing.rs:310-318) ----
@pytest.mark.parametrize("name,path_samples", [("config1", 2), ("config2", 2), ("config2", 3), ("config5", 2), ("config4", 2)])
def test_path_samples_greater_than_one(gpu_ctx, orc, name, path_samples):
    """The library routes path_samples != 1 to the recursive estimator (MI_VARIANT_RECURSIVE).  It nests the
    products exactly as the reference does, so the f32 image equals the oracle's bit for bit."""
    sc = {"config1": lambda: scenes.config1(64, 64, 4, 4), "config2": lambda: scenes.config2(96, 64, 4, 4),
          "config4": lambda: scenes.config4(64, 48, 4, 3, tex_size=64), "config5": lambda: scenes.config5(64, 48, 4, 5)}[name]()
    sc.camera.path_samples = path_samples
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    f32, u8, sig, _ = gpu_ctx.render(sc.camera, seed=3, want_sig=True)
    r32, r8, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=3)
    assert np.array_equal(sig, rsig)
    assert np.array_equal(f32, r32)
    assert int(np.abs(u8.astype(int) - r8.astype(int)).max()) <= 1


@pytest.mark.parametrize("name", ["config2", "config5", "head"])
def test_recursive_estimator_is_bit_identical_to_the_oracle(gpu_ctx, orc, name):
    """path_samples == 1 through MI_VARIANT_RECURSIVE: an independent check of every device function — not
    only the decisions (signatures) but the f32 radiance itself, bit for bit — and of the forward-accumulating
    default pipeline against it (same paths, radiance within the documented tolerance)."""
    sc = {"config2": lambda: scenes.config2(160, 96, 16, 10), "config5": lambda: scenes.config5(96, 64, 16, 50),
          "head": lambda: scenes.head_scene(64, 64, 4, 10)}[name]()
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    f32, _, sig, _ = gpu_ctx.render(sc.camera, seed=11, want_u8=False, want_sig=True, variant=abi.MI_VARIANT_RECURSIVE)
    r32, _, rsig, _ = orc.OracleScene(flat).render(sc.camera, seed=11, want_u8=False)
    assert np.array_equal(sig, rsig)
    assert np.array_equal(f32, r32)
    d32, _, dsig, _ = gpu_ctx.render(sc.camera, seed=11, want_u8=False, want_sig=True)
    assert np.array_equal(dsig, sig)
    assert float((np.abs(d32.astype(np.float64) - f32) / np.maximum(1.0, np.abs(f32))).max()) <= 2e-5
