"""Hand-built bakes (mean, second moments, per-texel counts) and centre tables for lightmap_select / lightmap_gather / lightmap_merge and
the finish with counts, shared by the host tests (which check what the helpers must do with them and that they notice mutants) and the
GPU tests (which ask the kernels for the helpers' bits on every one).  They are variance_batteries.py's cube and ragged tables with a
counts plane.

A battery is (name, image, m2, counts, points, normals, target_rel, target_abs): two [H, W, 3] float32 planes, an [H, W] uint32 plane, the
two guide tables and the two targets of lightmap_select.  Everything is built on the host from numpy; nothing here is ever fed anything
the GPU made.  The arrays are cached and read-only.

Targets.  The tables' moments give a per-sample standard deviation of rel * |value| * u, u in [0.5, 1.5) (variance_batteries.moments_for),
so the standard error of a texel's mean over its luminance is about rel * u / sqrt(n) times a factor between 1 / sqrt(3) and 1 (the
2-norm over the 1-norm of three channels).  The targets below sit inside that range for the counts each table carries;
test_lightmap_adaptive_host.py checks on the CPU that every battery selects between 5 % and 95 % of its covered texels."""
import numpy as np

import finish_batteries as fb
import variance_batteries as vb
from finish_batteries import INF, bits  # noqa: F401  (re-exported for the tests)

_cache = {}
BLOCK_SIZES = [(31, 33), (32, 32), (25, 41), (3, 683)]        # W x H: 1023, 1024, 1025 and 2049 texels against the 1024-texel block
TILE_WIDTHS = [31, 32, 33, 65]                                # at 33 rows
SINGLE_COUNT = 7
MIXED_VALUES = np.uint32([0, 1, 2, 3, 5, 8, 16])
MIXED_P = [0.03, 0.03, 0.14, 0.2, 0.2, 0.2, 0.2]


def _frozen(a):
    a.setflags(write=False)
    return a


def counts_plane(kind, H, W, samples, seed):
    """uniform: the table's own sample count everywhere; single: SINGLE_COUNT everywhere; mixed: MIXED_VALUES drawn per texel, a few
    texels with 0 and 1 among them"""
    key = ("counts", kind, H, W, samples, seed)
    if key not in _cache:
        if kind == "uniform":
            c = np.full((H, W), samples, np.uint32)
        elif kind == "single":
            c = np.full((H, W), SINGLE_COUNT, np.uint32)
        else:
            c = np.random.default_rng(seed).choice(MIXED_VALUES, size=(H, W), p=MIXED_P).astype(np.uint32)
        _cache[key] = _frozen(c)
    return _cache[key]


def from_variance_battery(battery, kind, target_rel, target_abs=0.0):
    name, img, m2, S, P, N, _ = battery
    H, W = img.shape[:2]
    return (f"{name}-{kind}", img, m2, counts_plane(kind, H, W, S, 99 + H * W), P, N, float(target_rel), float(target_abs))


# the relative target per counts plane: the tables' rel is 0.3 (cube, S = 8) and 0.4 (ragged, S = 5)
CUBE_TARGETS = {"uniform": 0.075, "single": 0.08, "mixed": 0.12}
RAGGED_TARGETS = {"uniform": 0.13, "single": 0.11, "mixed": 0.15}


def cube_batteries():
    return [from_variance_battery(b, kind, CUBE_TARGETS[kind], 1e-3) for b in vb.cube_batteries(3, 0) for kind in ("uniform", "mixed", "single")]


def ragged_battery(W, H, kind="mixed"):
    return from_variance_battery(vb.ragged_battery(W, H), kind, RAGGED_TARGETS[kind], 1e-3)


def block_batteries():
    """Texel counts of 1023, 1024, 1025 and 2049: one short of the compaction block, the block, one over, two blocks and one texel"""
    return [ragged_battery(W, H, kind) for (W, H), kind in zip(BLOCK_SIZES, ("mixed", "uniform", "mixed", "single"))]


def tile_batteries():
    return [ragged_battery(W, 33, "mixed") for W in TILE_WIDTHS]


def all_batteries():
    seen, out = set(), []
    for b in cube_batteries() + block_batteries() + tile_batteries() + [ragged_battery(33, 33, "uniform"), ragged_battery(33, 33, "single")]:
        if b[0] not in seen:
            seen.add(b[0])
            out.append(b)
    return out


def nothing_selected(battery):
    """target_abs = +inf: no texel's error exceeds it, not even an infinite one"""
    return (battery[0] + "-none",) + battery[1:6] + (0.0, INF)


def everything_noisy_selected(battery):
    """Both targets zero: every covered texel whose blurred variance is above zero is selected, and no other"""
    return (battery[0] + "-all",) + battery[1:6] + (0.0, 0.0)


def zero_variance_battery():
    """variance_batteries' two-colour table with m2 == mean * mean exactly: V = 0 everywhere, so with both targets zero the error EQUALS
    the threshold on every texel: `>` selects none of them, `>=` all"""
    name, img, m2, S, P, N, _ = vb.zero_variance_battery()
    H, W = img.shape[:2]
    return ("zero-variance-adaptive", img, m2, counts_plane("uniform", H, W, S, 0), P, N, 0.0, 0.0)


def extreme_batteries():
    noisy = ragged_battery(33, 33, "mixed")
    return [nothing_selected(noisy), everything_noisy_selected(noisy), zero_variance_battery()]


def round_for(battery, index, round_samples=4, seed=5):
    """A made-up refinement round for the texels of `index`: (mean', m2') [ch * cw, 3] with cw = 7, values near the texel's own"""
    _, img, m2 = battery[:3]
    n = int(np.size(index))
    slots = (n + 6) // 7 * 7
    rng = np.random.default_rng(seed + n)
    mean = np.zeros((slots, 3), np.float32)
    m2r = np.zeros((slots, 3), np.float32)
    ok = np.asarray(index) < img.shape[0] * img.shape[1]
    t = np.asarray(index)[ok].astype(np.int64)
    mean[:n][ok] = img.reshape(-1, 3)[t] * rng.uniform(0.8, 1.2, (t.size, 3)).astype(np.float32)
    m2r[:n][ok] = m2.reshape(-1, 3)[t] * rng.uniform(0.8, 1.2, (t.size, 3)).astype(np.float32)
    return mean, m2r
