"""Directional lightmaps on the host: the numpy definitions lightmap_finish_sh and lightmap_sh_eval against what they must agree with
(lightmap_finish plane by plane, probe_volume_sample on a one-probe volume), the constants of the bake's definition against a constant
field, and the Python-side refusals of the three calls.  No GPU and no library call."""
import numpy as np
import pytest

from cs397raytracingsp22_amd import (Camera, Context, Scene, abi, check_finish_sh_tables, check_sh_eval, lightmap_finish, lightmap_finish_sh,
                                     lightmap_sh_eval, probe_volume_sample, sh9_basis, sh9_irradiance)

import finish_batteries as fb
from finish_batteries import CUBE_SIZES, INF, bits, cube_noisy, cube_paint, cube_table, islands_battery, plane_battery, reach_equal_battery, two_halves

# nine distinct per-plane factors, none a power of two times another: a channel mix-up changes bits
PLANE_SCALE = np.float32([1.0, -0.7, 0.3, 1.9, -0.11, 0.57, -2.3, 0.013, 5.1])


def sh_records(image):
    """[H, W, 9, 3] f32: plane k is `image` times PLANE_SCALE[k] (one rounding)"""
    return np.ascontiguousarray((image[:, :, None, :] * PLANE_SCALE[None, None, :, None]).astype(np.float32))


def sh_batteries():
    """(name, sh, points, normals, params) for the two identities: the tables of tests/finish_batteries.py with 27 channels"""
    out = []
    for W, H in CUBE_SIZES:
        P, N, _ = cube_table(W, H)
        out.append((f"cube-flat-{W}x{H}", sh_records(cube_paint(W, H)), P, N, dict(levels=3, normal_power_log2=5, sigma_color=3.0, dilate=2)))
        out.append((f"cube-noisy-{W}x{H}", sh_records(cube_noisy(W, H)), P, N, dict(levels=3, normal_power_log2=5, sigma_color=6.0, dilate=2)))
    img, P, N = two_halves()
    out.append(("two-halves-colour", sh_records(img), P, N, dict(levels=3, normal_power_log2=5, sigma_color=0.5, dilate=0)))
    img, P, N = two_halves(gap=(0.0, 0.0, 1.0))
    out.append(("two-halves-plane", sh_records(img), P, N, dict(levels=2, normal_power_log2=1, sigma_plane=0.05, reach=1.5, sigma_color=2.0,
                                                                 dilate=1)))
    for name, img, P, N, params in (reach_equal_battery(), plane_battery(0.05), islands_battery()):
        out.append((name, sh_records(img), P, N, params))
    return out


BATTERIES = sh_batteries()


@pytest.mark.parametrize("battery", BATTERIES, ids=[b[0] for b in BATTERIES])
def test_plane_zero_is_lightmap_finish_of_plane_zero(battery):
    _, sh, P, N, params = battery
    out, valid = lightmap_finish_sh(sh, P, N, **params)
    ref, ref_valid = lightmap_finish(sh[:, :, 0, :], P, N, **params)
    assert out.shape == sh.shape and out.dtype == np.float32 and valid.dtype == bool
    assert np.array_equal(bits(out[:, :, 0, :]), bits(ref)) and np.array_equal(valid, ref_valid)
    covered = N.any(axis=-1)
    assert not bits(out)[~valid].any()                                  # +0.0 in all 27 channels of a texel nothing reached
    if params["levels"] and covered.sum() > 10:                         # the other planes are not copies of plane 0
        assert not np.array_equal(bits(out[:, :, 1, :]), bits(ref))


@pytest.mark.parametrize("battery", BATTERIES, ids=[b[0] for b in BATTERIES])
def test_without_the_colour_weight_every_plane_is_lightmap_finish_of_that_plane(battery):
    _, sh, P, N, params = battery
    params = dict(params, sigma_color=INF)
    out, valid = lightmap_finish_sh(sh, P, N, **params)
    for k in range(9):
        ref, ref_valid = lightmap_finish(sh[:, :, k, :], P, N, **params)
        assert np.array_equal(bits(out[:, :, k, :]), bits(ref)), k
        assert np.array_equal(valid, ref_valid)


def test_the_colour_weight_comes_from_plane_zero_only():
    """With a finite sigma_color a plane k > 0 is NOT lightmap_finish of that plane (whose colour distance would be its own): the
    weights are plane 0's.  And scaling the planes k > 0 scales their result exactly (a power of two), leaving plane 0's bits."""
    W, H = CUBE_SIZES[1]
    P, N, _ = cube_table(W, H)
    sh = sh_records(cube_noisy(W, H))
    params = dict(levels=2, normal_power_log2=5, sigma_color=2.0, dilate=1)
    out, _ = lightmap_finish_sh(sh, P, N, **params)
    own, _ = lightmap_finish(sh[:, :, 6, :], P, N, **params)
    assert not np.array_equal(bits(out[:, :, 6, :]), bits(own))
    sh4 = sh.copy()
    sh4[:, :, 1:, :] *= np.float32(4.0)
    out4, _ = lightmap_finish_sh(sh4, P, N, **params)
    assert np.array_equal(bits(out4[:, :, 0, :]), bits(out[:, :, 0, :]))
    assert np.array_equal(bits(out4[:, :, 1:, :]), bits(out[:, :, 1:, :] * np.float32(4.0)))


def test_finish_with_no_pass_is_the_masked_copy():
    W, H = CUBE_SIZES[0]
    P, N, covered = cube_table(W, H)
    sh = sh_records(cube_noisy(W, H)) + np.float32(7.0)                 # rubbish in the empty texels too
    out, valid = lightmap_finish_sh(sh, P, N, levels=0, dilate=0)
    assert np.array_equal(valid, covered)
    assert np.array_equal(bits(out)[covered], bits(sh)[covered]) and not bits(out)[~covered].any()


# ---------------------------------------------------------------- mutants of the blocks shared with lightmap_finish
def same_bits(x, y):
    return np.array_equal(bits(x[0]), bits(y[0])) and np.array_equal(x[1], y[1])


def test_unmutated_copy_is_the_helper():
    copy = fb.mutant(lightmap_finish_sh, fb.FINISH_BLOCKS, "for dy, dx in _LMF_TAPS:", "for dy, dx in _LMF_TAPS:")
    for _, sh, P, N, params in BATTERIES:
        assert same_bits(copy(sh, P, N, **params), lightmap_finish_sh(sh, P, N, **params))


@pytest.mark.parametrize("name", list(fb.LEVEL_AND_DILATION_MUTANTS))
def test_batteries_notice(name):
    """A slip in the level or the dilation that lightmap_finish's batteries notice does not pass the 27-channel form's either"""
    wrong = fb.mutant(lightmap_finish_sh, fb.FINISH_BLOCKS, *fb.LEVEL_AND_DILATION_MUTANTS[name])
    noticed = [b[0] for b in BATTERIES if not same_bits(wrong(*b[1:4], **b[4]), lightmap_finish_sh(*b[1:4], **b[4]))]
    print(f"{name}: noticed by {noticed}")
    assert noticed


# ---------------------------------------------------------------- evaluation
def _records_and_normals(n, seed):
    rng = np.random.default_rng(seed)
    sh = (rng.standard_normal((n, 9, 3)) * np.float32([2.0] + [1.0] * 3 + [0.5] * 5)[None, :, None]).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    nrm[::7] *= np.float32(1e-3)                                        # not normalised: only the direction matters
    nrm[3::11] = 0.0                                                    # empty texels, either sign of zero
    nrm[5::13] = -0.0
    nrm[::17, 1] = 0.0                                                  # normals in a coordinate plane
    return sh, nrm


def test_eval_equals_a_one_probe_volume_bit_for_bit():
    sh, nrm = _records_and_normals(300, 5)
    E = lightmap_sh_eval(sh, nrm)
    assert E.shape == (300, 3) and E.dtype == np.float32
    rng = np.random.default_rng(6)
    pts = rng.uniform(-3.0, 3.0, (300, 3)).astype(np.float32)           # inside and outside the box: one probe serves every point
    empty = ~nrm.any(axis=-1)
    assert 20 < empty.sum() < 100
    for i in range(300):
        ref, w = probe_volume_sample((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (1, 1, 1), sh[i:i + 1], pts[i:i + 1], nrm[i:i + 1])
        assert np.array_equal(bits(E[i]), bits(ref[0])), i
        assert float(w[0]) == (0.0 if empty[i] else 1.0)
    assert not bits(E)[empty].any()                                     # +0.0


def test_eval_agrees_with_sh9_irradiance():
    """the f32 chain against the float64 dot product with the exact cosine-lobe factors: K_k is A_l times the basis constant"""
    sh, nrm = _records_and_normals(200, 8)
    live = nrm.any(axis=-1)
    E = lightmap_sh_eval(sh, nrm)[live]
    ref = sh9_irradiance(sh[live], nrm[live].astype(np.float64))
    mass = (np.abs(sh[live].astype(np.float64)) * np.abs(sh9_basis(nrm[live].astype(np.float64)))[..., None] * np.pi).sum(axis=-2)
    assert float((np.abs(E - ref) / np.maximum(1.0, mass)).max()) <= 2e-6


def test_eval_takes_an_atlas_with_its_normal_table():
    W, H = CUBE_SIZES[0]
    _, N, covered = cube_table(W, H)
    sh = sh_records(cube_noisy(W, H))
    E = lightmap_sh_eval(sh, N)
    assert E.shape == (H, W, 3) and not bits(E)[~covered].any()
    assert np.array_equal(bits(E), bits(lightmap_sh_eval(sh, N[None])))                 # lightmap_texels' [1, H, W, 3]
    assert np.array_equal(bits(E.reshape(-1, 3)), bits(lightmap_sh_eval(sh.reshape(-1, 9, 3), N.reshape(-1, 3))))


@pytest.mark.parametrize("normal", [(0.0, 1.0, 0.0), (0.0, 0.0, -1.0), (1.0, 2.0, -0.5), (-0.3, -0.2, 0.9)])
def test_constant_radiance_gives_pi(normal):
    """The bake's definition on a constant field of radiance 1: directions uniform over the hemisphere about n (pdf 1 / (2 pi)),
    c_k = (2 pi / S) sum_s Y_k(u_s), E(n) = sum_k A_l c_k Y_k(n).  Its expectation is exactly pi: the order-2 expansion of the clamped
    cosine is 1/4 + cos/2 + (5/16) (3 cos^2 - 1) / 2..., and over the hemisphere the constant and the linear term integrate to pi / 2
    each while the l = 2 term integrates to zero.  E is the mean of the per-sample values e_s = 2 pi sum_k A_l Y_k(u_s) Y_k(n), so its
    standard error is their own spread / sqrt(S).  A 4 pi left in the place of 2 pi gives 2 pi; a swapped K_k moves it by tens of
    standard errors."""
    from cs397raytracingsp22_amd.tracing import SH9_COSINE
    S = 20000
    n = np.float64(normal) / np.linalg.norm(np.float64(normal))
    u = np.random.default_rng(11).standard_normal((S, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    u = np.where((u @ n)[:, None] < 0, -u, u)                           # reflected into the hemisphere about n: still uniform there
    Y = sh9_basis(u)                                                     # [S, 9]
    c = (2.0 * np.pi / S) * Y.sum(axis=0)                                # radiance 1 in every channel
    e_s = 2.0 * np.pi * (Y * (SH9_COSINE * sh9_basis(n))[None, :]).sum(axis=-1)
    E = float(sh9_irradiance(c[:, None], n)[0])
    assert abs(E - float(e_s.mean())) <= 1e-9                            # the same number, two ways
    stderr = float(e_s.std(ddof=1) / np.sqrt(S))
    print(f"n = {normal}: E = {E:.5f}, pi = {np.pi:.5f}, standard error {stderr:.5f}")
    assert 1e-4 < stderr < 0.05
    assert abs(E - np.pi) <= 5.0 * stderr
    E32 = lightmap_sh_eval(np.repeat(c[:, None], 3, axis=1).astype(np.float32), np.float32(normal))      # the f32 definition, any length of n
    assert E32.shape == (3,) and float(np.abs(E32 - E).max()) <= 1e-5 * np.pi


# ---------------------------------------------------------------- the layers above
def test_abi_lists_the_seven_calls():
    import ctypes as C
    lib = abi.load()
    for name, n_args in (("mi_render_points_sh", 11), ("mi_render_points_sh_device", 14), ("mi_bake_lightmap_sh", 12),
                         ("mi_lightmap_finish_sh", 14), ("mi_lightmap_finish_sh_device", 15), ("mi_lightmap_sh_eval", 5),
                         ("mi_lightmap_sh_eval_device", 6)):
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == n_args, name


def _cam(w=6, h=5, aa=4):
    return Camera(screen_width=w, screen_height=h, aa_sample_count=aa, path_depth=4, max_trace_dist=100.0, gamma=2.0)


def test_python_refusals_come_before_any_library_call():
    ctx = Context.__new__(Context)                        # no mi_ctx_create: any library call would fail on the missing handle
    t = np.zeros((4, 5, 6, 3), np.float32)
    with pytest.raises(ValueError):
        Context.render_points_sh(ctx, _cam(), t[:2], t[:2])                              # rows is neither 1 nor aa_sample_count
    with pytest.raises(ValueError):
        Context.render_points_sh(ctx, _cam(), t, t[:, :, :5])                            # two shapes
    with pytest.raises(ValueError):
        Context.render_points_sh(ctx, _cam(), t.astype(np.float64), t)                   # not float32
    from cs397raytracingsp22_amd import objload
    from finish_batteries import cube_mesh
    mesh = cube_mesh()
    with pytest.raises(ValueError):                                                      # a malformed mesh
        Context.bake_lightmap_sh(ctx, _cam(), objload.Mesh(mesh.positions, mesh.normals[:-3], mesh.texcoords, mesh.indices))
    sh = np.zeros((5, 6, 9, 3), np.float32)
    g = np.zeros((5, 6, 3), np.float32)
    for bad in ((sh[..., :2], g, g), (sh.reshape(5, 6, 27), g, g), (sh, g[:4], g), (sh, g, g[:, :5]), (np.zeros((0, 6, 9, 3), np.float32), g[:0], g[:0])):
        with pytest.raises(ValueError):
            Context.lightmap_finish_sh(ctx, *bad)
        with pytest.raises(ValueError):
            lightmap_finish_sh(*bad)
    for kw in (dict(levels=9), dict(normal_power_log2=8), dict(dilate=257), dict(sigma_color=0.0), dict(reach=-1.0), dict(sigma_plane=float("nan"))):
        with pytest.raises(ValueError):
            lightmap_finish_sh(sh, g, g, **kw)
    assert [a.shape for a in check_finish_sh_tables(sh, g[None], g[None])] == [(5, 6, 9, 3), (5, 6, 3), (5, 6, 3)]
    for bad in ((sh[..., :2], g), (sh, g[:4]), (sh.reshape(-1, 9, 3), g), (sh, g[..., :2]), (sh[0, 0, 0], g[0, 0])):
        with pytest.raises(ValueError):
            Context.lightmap_sh_eval(ctx, *bad)
        with pytest.raises(ValueError):
            lightmap_sh_eval(*bad)
    S, N, shape = check_sh_eval(sh, g)
    assert S.shape == (30, 9, 3) and N.shape == (30, 3) and shape == (5, 6)
    assert lightmap_sh_eval(sh[:0].reshape(0, 9, 3), g[:0].reshape(0, 3)).shape == (0, 3)                # no point is no error


def test_scene_bake_refuses_what_a_directional_bake_does_not_combine_with():
    sc = Scene(_cam(), [])
    for kw in (dict(adaptive=dict(round_samples=4, max_rounds=1, target_rel=0.1, target_abs=0.0)), dict(finish=dict(variance=True))):
        with pytest.raises(ValueError):
            sc.bake_lightmap(object(), 6, 5, 4, directional=True, **kw)
