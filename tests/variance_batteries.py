"""Hand-built bakes (mean, second moments, sample count) and guide tables for lightmap_finish_var / mi_lightmap_finish_var, shared by the
host tests (which check what the helper must do with them and that they notice mutants of it) and the GPU tests (which ask the kernels
for the helper's bits on every one).  They build on finish_batteries.py.

A battery is (name, image, m2, samples, points, normals, params): three [H, W, 3] float32 arrays and the sample count they stand for,
the two guide tables and the keyword arguments of lightmap_finish_var.  Everything is built on the host from numpy; nothing here is ever
fed anything the GPU made.  The arrays are cached and read-only."""
import numpy as np

import finish_batteries as fb
from finish_batteries import BASE, INF, bits, flat_table  # noqa: F401  (re-exported for the tests)

_cache = {}
NOISE_SEEDS = (7, 8, 9)
NOISE_SAMPLES = 16
NOISE_LEVELS = 4
NOISY_REGION = (slice(8, 56), slice(8, 40))             # rows 8 .. 55 x columns 8 .. 39
STEP_REGION = (slice(8, 56), slice(68, 76))             # rows 8 .. 55 x columns 68 .. 75: the step lies between columns 71 and 72
FIXED_SIGMAS = (0.03, 0.1, 0.3, 1.0, 3.0, 10.0)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def moments_for(img, samples, rel, seed):
    """Second moments that give texel values a standard deviation of rel * |value| * u per sample, u uniform in [0.5, 1.5) per value:
    m2 = mean^2 + sd^2 (S - 1) / S, rounded once to f32 (so the variance the filter recovers is that up to f32 cancellation)"""
    u = np.random.default_rng(seed).uniform(0.5, 1.5, img.shape)
    sd = rel * np.abs(img.astype(np.float64)) * u
    return (img.astype(np.float64) ** 2 + sd * sd * (samples - 1) / samples).astype(np.float32)


def from_finish_battery(battery, samples=8, rel=0.3, tag="", **override):
    """A finish battery with moments: a quiet-to-noisy spread of variances over its own image.  Names are unique per parameter set:
    `tag` tells apart two batteries made from one finish battery."""
    name, img, P, N, params = battery
    key = ("fb", name, samples, rel)
    if key not in _cache:
        _cache[key] = _frozen(moments_for(img, samples, rel, 4242 + len(name)))[0]
    kw = dict(params)
    kw.pop("sigma_color", None)                          # the fixed filter's colour sigma has another meaning: standard errors here
    kw.update(dict(sigma_color=6.0, color_floor=1e-3), **override)
    return (f"var-{name}{tag}", img, _cache[key], samples, P, N, kw)


def cube_batteries(levels=3, dilate=0, **override):
    return [from_finish_battery(b, **override) for b in fb.cube_batteries(levels, dilate)]


def ragged_battery(W, H, levels=4, dilate=2):
    """finish_batteries' ragged table (a quarter empty, finite sigma_plane and reach, a noisy image) with moments: every weight in play"""
    return from_finish_battery(fb.ragged_battery(W, H, levels, dilate), samples=5, rel=0.4, sigma_color=3.0, color_floor=0.01)


def colour_off_batteries():
    """The noisy cube tables at 3 levels with color_floor = inf: lightmap_finish(sigma_color=inf)'s image, bit for bit"""
    return [from_finish_battery(b, tag="-colour-off", color_floor=INF) for b in fb.cube_batteries(3, 0)[1::2]]


def zero_variance_battery():
    """A two-colour flat table painted powers of two times BASE, m2 == mean * mean exactly (the squares of such values are exact): V = 0
    everywhere, den = color_floor, so a tap of the other colour weighs nothing and one of the texel's own colour weighs w exactly"""
    img, P, N = fb.two_halves()
    m2 = img * img
    assert np.array_equal(m2.astype(np.float64), img.astype(np.float64) ** 2)
    return ("zero-variance", img, _frozen(m2)[0], 4, P, N, dict(levels=4, normal_power_log2=5, sigma_color=8.0, color_floor=1e-6, dilate=0))


PROPAGATION_V0 = np.float32(0.75)


def propagation_battery():
    """A constant colour 1 with m2 = 1.25 and S = 2: v_c = 0.25, V0 = 0.75 everywhere; a flat table, so every weight but h is 1"""
    W, H = 15, 13
    P, N = flat_table(W, H)
    img = np.ones((H, W, 3), np.float32)
    m2 = np.full((H, W, 3), 1.25, np.float32)
    return ("propagation", *_frozen(img, m2), 2, *_frozen(P, N), dict(levels=1, normal_power_log2=5, sigma_color=8.0, color_floor=1e-6, dilate=0))


def noise_truth():
    truth = np.empty((64, 96, 3), np.float32)
    truth[:, :48] = (1.0, 0.5, 2.0)
    truth[:, 48:72] = 0.5
    truth[:, 72:] = 0.625
    return truth


def noise_battery(seed, sigma_color=16.0, color_floor=1e-6):
    """The two-noise-level bake: flat 96 x 64, S = 16; the left half a flat colour with per-sample sd 0.5, the right half quiet (sd 0.01)
    with a faint 0.125 step.  Means and moments are summed in sample order in f32, as the bake does."""
    key = ("noise", seed)
    if key not in _cache:
        H, W, S = 64, 96, NOISE_SAMPLES
        z = np.random.default_rng(seed).standard_normal((S, H, W, 3)).astype(np.float32)
        sd = np.where(np.arange(W) < 48, np.float32(0.5), np.float32(0.01)).astype(np.float32)
        samples = noise_truth()[None] + z * sd[None, None, :, None]
        mean = np.zeros((H, W, 3), np.float32)
        m2 = np.zeros((H, W, 3), np.float32)
        for s in range(S):
            mean = mean + samples[s]
            m2 = m2 + samples[s] * samples[s]
        P, N = flat_table(W, H)
        _cache[key] = _frozen(mean / np.float32(S), m2 / np.float32(S), P, N)
    mean, m2, P, N = _cache[key]
    return (f"noise-{seed}", mean, m2, NOISE_SAMPLES, P, N,
            dict(levels=NOISE_LEVELS, normal_power_log2=5, sigma_color=sigma_color, color_floor=color_floor, dilate=0))


def region_errors(out):
    """(noisy region, step region) mean absolute error against the truth"""
    err = np.abs(out.astype(np.float64) - noise_truth())
    return float(err[NOISY_REGION].mean()), float(err[STEP_REGION].mean())


def edge_batteries():
    """1 x 1, an all-empty table, and levels = 0 (the masked copy and the initial variance) with dilation"""
    _, one, empty = fb.limiting_batteries()
    W, H = fb.CUBE_SIZES[0]
    P, N, _ = fb.cube_table(W, H)
    copy = ("cube-noisy-copy", fb.cube_noisy(W, H), P, N, dict(levels=0, normal_power_log2=5, dilate=3))
    return [from_finish_battery(one), from_finish_battery(empty), from_finish_battery(copy)]


def all_batteries(cube_levels=3, cube_dilate=0):
    """Every battery the mutants and the kernels are held against (the noise battery once: seed 7)"""
    return (cube_batteries(cube_levels, cube_dilate) + colour_off_batteries() +
            [zero_variance_battery(), propagation_battery(), noise_battery(NOISE_SEEDS[0]), ragged_battery(33, 33),
             from_finish_battery(fb.reach_equal_battery())] + edge_batteries())
