"""lightmap_finish_var, the host helper that defines mi_lightmap_finish_var: what it must do with the batteries of variance_batteries.py,
that those batteries notice one-token mutants of it, and the refusals of the five new entry points that need no device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from cs397raytracingsp22_amd import abi, lightmap_finish, lightmap_finish_var, tracing

import finish_batteries as fb
import variance_batteries as vb
from variance_batteries import INF, bits


def run(battery, finish=lightmap_finish_var, **override):
    _, img, m2, samples, P, N, params = battery
    return finish(img, m2, samples, P, N, **{**params, **override})


_ref = {}


def reference(battery):
    if battery[0] not in _ref:
        _ref[battery[0]] = run(battery)
    return _ref[battery[0]]


# ---------------------------------------------------------------- colour weight off
@pytest.mark.parametrize("k", [0, 1])
def test_colour_weight_off_is_the_fixed_filter(k):
    """color_floor = inf: 1 - dc / inf == 1, and the image is lightmap_finish(sigma_color=inf)'s bit for bit on both cube tables"""
    b = vb.colour_off_batteries()[k]
    _, img, m2, S, P, N, params = b
    assert params["levels"] == 3 and params["color_floor"] == INF
    out, var, valid = reference(b)
    want, want_valid = lightmap_finish(img, P, N, levels=3, normal_power_log2=params["normal_power_log2"], sigma_color=INF, dilate=params["dilate"])
    assert np.array_equal(valid, want_valid)
    assert int((bits(out) != bits(want)).sum()) == 0
    assert (var[valid] > 0).any() and not bits(var)[~valid].any()


# ---------------------------------------------------------------- zero variance
def test_zero_variance_keeps_every_bit():
    b = vb.zero_variance_battery()
    out, var, valid = reference(b)
    assert b[6]["levels"] == 4 and valid.all()
    assert np.array_equal(bits(out), bits(b[1]))
    assert not bits(var).any()
    assert len(np.unique(b[1][..., 0])) == 2


# ---------------------------------------------------------------- propagation
def test_variance_propagates_by_the_kernels_square_sum():
    """One level, all weights 1: V' = V0 sum(h^2) / sum(h)^2 = V0 (70/256)^2 for the separable B3 kernel, within 4 ulp"""
    b = vb.propagation_battery()
    _, var0, _ = run(b, levels=0)
    assert np.array_equal(var0, np.full(var0.shape, vb.PROPAGATION_V0))
    out, var, _ = reference(b)
    assert np.array_equal(bits(out), bits(b[1]))
    want = np.float32(float(vb.PROPAGATION_V0) * (70.0 / 256.0) ** 2)
    inner = var[2:-2, 2:-2]
    ulps = np.abs(bits(inner).astype(np.int64) - int(bits(want).item()))
    print(f"interior variance {inner[0, 0]!r} against {want!r}: at most {int(ulps.max())} ulp")
    assert int(ulps.max()) <= 4
    assert (var[0, :] > want).all()                       # at the border fewer taps: less averaging


# ---------------------------------------------------------------- the two-noise-level battery
@pytest.mark.parametrize("seed", vb.NOISE_SEEDS)
def test_two_noise_levels(seed):
    """The variance-guided weight denoises the noisy half to a tenth of the raw error AND does not hurt the faint step in the quiet half;
    no fixed sigma_color does both."""
    b = vb.noise_battery(seed)
    _, mean, m2, S, P, N, params = b
    assert S == 16 and params["levels"] == 4 and params["sigma_color"] == 16.0 and params["color_floor"] == 1e-6
    raw_noisy, raw_step = vb.region_errors(mean)
    out, _, _ = reference(b)
    noisy, step = vb.region_errors(out)
    print(f"seed {seed}: raw {raw_noisy:.4f} / {raw_step:.5f}; variance-guided {noisy:.4f} ({noisy / raw_noisy:.3f} x raw) / "
          f"{step:.5f} ({step / raw_step:.3f} x raw)")
    assert noisy <= 0.1 * raw_noisy
    assert step <= raw_step
    for sigma in vb.FIXED_SIGMAS:
        fixed, _ = lightmap_finish(mean, P, N, levels=4, normal_power_log2=5, sigma_color=sigma, dilate=0)
        f_noisy, f_step = vb.region_errors(fixed)
        print(f"    fixed sigma_color {sigma}: {f_noisy / raw_noisy:.3f} x raw / {f_step / raw_step:.3f} x raw")
        assert f_noisy > 0.1 * raw_noisy or f_step > raw_step, sigma


# ---------------------------------------------------------------- edges
def test_edges():
    one, empty, copy = vb.edge_batteries()
    out, var, valid = reference(one)
    assert out.shape == (1, 1, 3) and valid.all() and np.array_equal(bits(out), bits(one[1])) and var[0, 0] > 0
    out, var, valid = reference(empty)
    assert not valid.any() and not bits(out).any() and not bits(var).any()
    # levels = 0: the masked copy, the initial variance, and a dilation that leaves the variance of filled texels +0.0
    out, var, valid = reference(copy)
    _, img, m2, S, P, N, _ = copy
    covered = (N != 0).any(axis=-1)
    assert np.array_equal(bits(out)[covered], bits(img)[covered]) and valid.sum() > covered.sum()
    v3 = np.fmax(np.float32(0), m2 - img * img) / np.float32(S - 1)
    want = np.where(covered, (v3[..., 0] + v3[..., 1]) + v3[..., 2], np.float32(0))
    assert np.array_equal(bits(var), bits(want)) and not bits(var)[~covered].any()


def test_non_finite_texel_spoils_its_footprint_only():
    b = vb.cube_batteries(2, 2)[1]
    _, clean, m2, S, P, N, params = b
    covered = (N != 0).any(axis=-1)
    H, W = covered.shape
    ys, xs = np.nonzero(covered)
    k = int(np.argmin(np.maximum(np.abs(ys - H // 2), np.abs(xs - W // 2))))
    y0, x0 = int(ys[k]), int(xs[k])
    yy, xx = np.mgrid[0:H, 0:W]
    far = np.maximum(np.abs(yy - y0), np.abs(xx - x0)) > 2 * (2 ** 2 - 1) + 2 + 2
    assert far.sum() > 1000
    ref = reference(b)
    for which, value in ((0, np.nan), (1, np.inf)):           # (a NaN moment is swallowed by the fmaxf of the initial variance)
        dirty = [clean.copy(), m2.copy()]
        dirty[which][y0, x0] = value
        out, var, valid = lightmap_finish_var(dirty[0], dirty[1], S, P, N, **params)
        assert not np.isfinite(out).all() or not np.isfinite(var).all()
        assert np.array_equal(valid, ref[2]) and np.array_equal(bits(out)[far], bits(ref[0])[far]) and np.array_equal(bits(var)[far], bits(ref[1])[far])


def test_bad_arguments_are_refused():
    _, img, m2, S, P, N, _ = vb.propagation_battery()
    nan = float("nan")
    for bad in (dict(levels=9), dict(levels=-1), dict(normal_power_log2=8), dict(dilate=257), dict(sigma_plane=0.0), dict(sigma_plane=nan),
                dict(reach=-1.0), dict(reach=nan), dict(sigma_color=nan), dict(sigma_color=INF), dict(sigma_color=-0.5),
                dict(color_floor=0.0), dict(color_floor=nan), dict(color_floor=-1.0)):
        with pytest.raises(ValueError):
            lightmap_finish_var(img, m2, S, P, N, **bad)
    for samples in (1, 0, 65536):
        with pytest.raises(ValueError):
            lightmap_finish_var(img, m2, samples, P, N)
    with pytest.raises(ValueError):
        lightmap_finish_var(img, m2[:4], S, P, N)
    with pytest.raises(ValueError):
        lightmap_finish_var(img, m2, S, P[:4], N)
    with pytest.raises(ValueError):
        lightmap_finish_var(img[..., :2], m2[..., :2], S, P, N)
    # the limits themselves are legal
    lightmap_finish_var(img, m2, 2, P, N, levels=0, sigma_color=0.0, color_floor=INF, dilate=0)
    lightmap_finish_var(img, m2, 65535, P, N, levels=1, dilate=0)


# ---------------------------------------------------------------- mutants
MUTANTS = {
    "S for S - 1": fb.VARIANCE_MUTANTS["n for n - 1"],
    "w for w * w in sv": ("sv + (w * w) * vq", "sv + (w) * vq"),
    "sw for sw * sw": ("sv / (sw * sw)", "sv / (sw)"),
    "blur taken at step s": ("_lmv_blur(V, N, covered, 1) ", "_lmv_blur(V, N, covered, s) "),
    "den divided by s": ("den = sig_c0 * sd + floor", "den = (sig_c0 * sd + floor) / f32(s)"),
    "blur includes empty neighbours": fb.VARIANCE_MUTANTS["blur includes empty neighbours"],
    "variance read at p, not at q": ("vq = vpad[ys:ys + H, xs:xs + W]", "vq = V"),
    "blur's G3 flattened": ("G3 = (f32(0.25), f32(0.5), f32(0.25))", "G3 = (f32(0.25), f32(0.25), f32(0.25))"),
    **fb.LEVEL_AND_DILATION_MUTANTS,
}


def mutant(old, new):
    return fb.mutant(lightmap_finish_var, fb.VAR_BLOCKS, old, new)


def same_bits(x, y):
    return np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(bits(x[1]), bits(y[1])) and np.array_equal(x[2], y[2])


def test_unmutated_copy_is_the_helper():
    copy = mutant("den = sig_c0 * sd + floor", "den = sig_c0 * sd + floor")
    for b in vb.all_batteries(3, 2):
        assert same_bits(run(b, copy), reference(b)), b[0]


@pytest.mark.parametrize("name", list(MUTANTS))
def test_batteries_notice(name):
    """At least one battery's output (image bits, variance bits or mask) differs between the helper and the mutant."""
    wrong = mutant(*MUTANTS[name])
    noticed = [b[0] for b in vb.all_batteries(3, 2) if not same_bits(run(b, wrong), reference(b))]
    print(f"{name}: noticed by {noticed}")
    assert noticed


# ---------------------------------------------------------------- the library's refusals that need no device
def test_finish_var_refusals_come_before_the_context():
    lib = abi.load()
    _, img, m2, S, P, N, _ = vb.ragged_battery(31, 33)
    H, W = img.shape[:2]
    out = np.full((H, W, 3), -7.0, np.float32)
    var = np.full((H, W), -7.0, np.float32)
    valid = np.full((H, W), 9, np.uint8)
    nan = float("nan")

    def call(device, w=W, h=H, image=img.ctypes.data, m2_=m2.ctypes.data, samples=S, points=P.ctypes.data, normals=N.ctypes.data, levels=3,
             npow=5, sigma_plane=INF, reach=INF, sigma_color=8.0, color_floor=1e-6, dilate=4, out_image=out.ctypes.data):
        args = (None, w, h, image, m2_, samples, points, normals, levels, npow, sigma_plane, reach, sigma_color, color_floor, dilate,
                out_image, var.ctypes.data, valid.ctypes.data)
        rc = lib.mi_lightmap_finish_var_device(*args, None) if device else lib.mi_lightmap_finish_var(*args)
        return rc, lib.mi_last_error().decode()

    refused = [(dict(image=None), "required"), (dict(m2_=None), "required"), (dict(points=None), "required"), (dict(normals=None), "required"),
               (dict(out_image=None), "required"), (dict(w=0), "width"), (dict(h=0), "width"), (dict(w=32769), "width"), (dict(h=32769), "width"),
               (dict(levels=9), "levels"), (dict(npow=8), "normal_power_log2"), (dict(dilate=257), "dilate"),
               (dict(samples=1), "samples"), (dict(samples=0), "samples"), (dict(samples=65536), "samples"),
               (dict(sigma_plane=nan), "sigma_plane"), (dict(sigma_plane=0.0), "sigma_plane"), (dict(sigma_plane=-1.0), "sigma_plane"),
               (dict(reach=nan), "reach"), (dict(reach=0.0), "reach"), (dict(reach=-INF), "reach"),
               (dict(sigma_color=nan), "sigma_color"), (dict(sigma_color=INF), "sigma_color"), (dict(sigma_color=-0.5), "sigma_color"),
               (dict(color_floor=nan), "color_floor"), (dict(color_floor=0.0), "color_floor"), (dict(color_floor=-1.0), "color_floor")]
    for device in (False, True):
        for kw, word in refused:
            rc, msg = call(device, **kw)
            assert rc == abi.MI_ERR_INVALID and word in msg and "ctx" not in msg, (kw, device, msg)
        # legal arguments (the limits included) get as far as the missing context
        for kw in (dict(), dict(levels=8, npow=7, dilate=256, samples=2), dict(samples=65535, sigma_color=0.0, color_floor=INF)):
            rc, msg = call(device, **kw)
            assert rc == abi.MI_ERR_INVALID and msg == "ctx is NULL", (kw, device, msg)
    # the device form's overlap refusals, too, need no device: the host arrays stand in for device memory
    base, plane = img.ctypes.data, H * W * 12
    for kw, word in ((dict(out_image=base), "out_image"), (dict(out_image=base + plane - 4), "out_image"),
                     (dict(out_image=m2.ctypes.data + 8), "out_image")):
        rc, msg = call(True, **kw)
        assert rc == abi.MI_ERR_INVALID and "overlap" in msg and word in msg, (kw, msg)
    args = (None, W, H, img.ctypes.data, m2.ctypes.data, S, P.ctypes.data, N.ctypes.data, 3, 5, INF, INF, 8.0, 1e-6, 4, out.ctypes.data)
    for bad_var in (P.ctypes.data, N.ctypes.data + plane - 4):
        rc = lib.mi_lightmap_finish_var_device(*args, bad_var, valid.ctypes.data, None)
        assert rc == abi.MI_ERR_INVALID and "out_var overlaps" in lib.mi_last_error().decode()
    assert (out == -7.0).all() and (var == -7.0).all() and (valid == 9).all()


def test_moments_refusals_without_a_device():
    """out_m2 is required and checked first; everything else is mi_render_points' / mi_bake_lightmap's, which begin at the context"""
    lib = abi.load()
    cam = tracing.Camera(screen_width=4, screen_height=3, aa_sample_count=2, path_depth=2).to_pod()
    opts = abi.mi_render_opts(seed=1, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=0, flags=0, max_state_bytes=0)
    t = np.zeros((3, 4, 3), np.float32)
    m2 = np.full((3, 4, 3), -7.0, np.float32)
    st = abi.mi_stats()
    mesh = abi.mi_mesh()
    rc = lib.mi_render_points_moments(None, C.byref(cam), C.byref(opts), t.ctypes.data, t.ctypes.data, 1, None, None, None, None, C.byref(st))
    assert rc == abi.MI_ERR_INVALID and "mi_render_points_moments: out_m2 is required" in lib.mi_last_error().decode()
    rc = lib.mi_bake_lightmap_moments(None, C.byref(cam), C.byref(opts), C.byref(mesh), 0, 0.0, None, None, None, None, None, C.byref(st))
    assert rc == abi.MI_ERR_INVALID and "mi_bake_lightmap_moments: out_m2 is required" in lib.mi_last_error().decode()
    rc = lib.mi_render_points_moments(None, C.byref(cam), C.byref(opts), t.ctypes.data, t.ctypes.data, 1, m2.ctypes.data, None, None, None,
                                      C.byref(st))
    assert rc == abi.MI_ERR_INVALID and lib.mi_last_error().decode() == "ctx is NULL"
    rc = lib.mi_render_points_moments_device(None, C.byref(cam), C.byref(opts), t.ctypes.data, t.ctypes.data, 1, 0, 2, None, m2.ctypes.data,
                                             None, None, None, C.byref(st))
    assert rc == abi.MI_ERR_INVALID and lib.mi_last_error().decode() == "ctx is NULL"
    rc = lib.mi_bake_lightmap_moments(None, C.byref(cam), C.byref(opts), C.byref(mesh), 0, 0.0, m2.ctypes.data, None, None, None, None,
                                      C.byref(st))
    assert rc == abi.MI_ERR_INVALID and lib.mi_last_error().decode() == "ctx is NULL"
    assert (m2 == -7.0).all()


def test_mirrors_name_the_new_calls():
    import os
    root = fb.ROOT
    hpp = open(os.path.join(root, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "bake_lightmap_moments(" in hpp and "finish_lightmap_var(" in hpp
    rs = open(os.path.join(root, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn bake_lightmap_moments(" in rs and "pub fn finish_lightmap_var(" in rs
    for name in ("render_points_moments", "render_points_moments_device", "bake_lightmap_moments", "lightmap_finish_var",
                 "lightmap_finish_var_device", "last_reduce_m2_ms"):
        assert callable(getattr(tracing.Context, name)), name
