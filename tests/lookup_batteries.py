"""Data shared by tests/test_lightmap_lookup_host.py and tests/test_gpu_lightmap_lookup.py: images, masks, uv points and normals aimed at
the decision edges of lightmap_sample / lightmap_sh_sample (tracing.py), the float64 restatement both are held to, and the cube scene
of the end-to-end test.  Nothing here needs a GPU.

Sizes (W x H): 1x1, 2x1, 1x2, 5x3, 8x8, 45x33 and the two strips 32768x1 and 1x32768 (the largest legal extent: 0.999 W leaves the last
texel only above W = 1000, and u W rounds by up to 2^-9 there).
Points per size: every texel centre, searched among the f32 neighbours of (x + 0.5) / W so that gx and gy are exact integers (all of them
at the power-of-two sizes; at 5, 3, 45 and 33 some centres have no such f32 and stand as the nearest one, marked inexact); the
half-texel grid u = k / 2W, v = 1 - j / 2H (every corner and every edge midpoint; on a strip three windows of it); the cross product of
the special coordinates {-0.0, 0, 1, 0.999 and its two f32 neighbours, -0.25, 1.75, +inf, -inf, NaN}; and, around every k / n, the f32
neighbours whose product with n rounds across the integer k from below and from above.
Masks per size: none, all valid, a checkerboard, the four parity classes (each leaves exactly one valid tap in a 2 x 2 footprint, in each
of the four positions as the footprint moves), all invalid, a checkerboard whose invalid texels hold NaN and inf ("poison": none of it may
reach an output), and an all-valid image with one NaN and one inf texel ("spoiled": it may reach only the taps that touch it)."""
import numpy as np

from cs397raytracingsp22_amd import Camera, Lambertian, Scene, StaticMesh, cgmath, scenes
from cs397raytracingsp22_amd import lightmap_sample, lightmap_sh_sample
from cs397raytracingsp22_amd.tracing import PV_K, _lml_axis

import finish_batteries as fb

f32 = np.float32
SIZES = ((1, 1), (2, 1), (1, 2), (5, 3), (8, 8), (45, 33), (32768, 1), (1, 32768))          # (W, H)
SMALL = SIZES[:6]
SPECIAL = np.array([-0.0, 0.0, 1.0, 0.999, np.nextafter(f32(0.999), f32(0)), np.nextafter(f32(0.999), f32(1)), -0.25, 1.75,
                    np.inf, -np.inf, np.nan], f32)
MASKS = ("none", "all", "checker", "parity00", "parity01", "parity10", "parity11", "all invalid", "poison", "spoiled")
COUNTS = (1, 255, 256, 257)
_cache = {}


def bits(a):
    """The bit patterns of an f32 array, every NaN as the one quiet NaN: which NaN an operation makes (its sign, its payload) is the
    processor's choice, not the definition's; everything else, infinities and signed zeros included, counts bit for bit"""
    a = np.ascontiguousarray(a, f32)
    b = a.view(np.uint32).copy()
    b[np.isnan(a)] = 0x7FC00000
    return b


def _frozen(a):
    a.setflags(write=False)
    return a


def _ulps(x, k):
    """the f32 k steps away from x (k of either sign)"""
    x = f32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


def _exact_centres(n, flip):
    """[(coordinate, exact)] of the n texel centres: the nearest f32 to (i + 0.5) / n (or to 1 less it when `flip`) or one of its
    neighbours up to 4 steps away, the first whose g = t n - 0.5 (t the coordinate, or 1 - it) is exactly i in f32; where none is
    (1 - v has v's spacing, too coarse for some i / n), the nearest f32 itself, marked inexact"""
    out = []
    for i in range(n):
        c = (i + 0.5) / n
        c = 1.0 - c if flip else c
        for k in (0, 1, -1, 2, -2, 3, -3, 4, -4):
            t = _ulps(c, k)
            g = ((f32(1.0) - t) if flip else t) * f32(n) - f32(0.5)
            if g == f32(i):
                out.append((t, True))
                break
        else:
            out.append((f32(c), False))
    return out


def _crossing(n, flip, ks):
    """Coordinates around m / n, m = k (where the nearest form's trunc decides) and m = k + 0.5 (where the bilinear form's floor does),
    k in ks, whose f32 product with n is m although the exact product lies below it ('up') or above it ('down'):
    ([coordinates], number of 'up', number of 'down').  Every neighbour up to 2 steps away is kept as a point."""
    pts, up, down = [], 0, 0
    for m in [k + h for k in ks for h in (0.0, 0.5) if k + h <= n]:
        c = m / n
        c = 1.0 - c if flip else c
        for s in range(-2, 3):
            t = _ulps(c, s)
            a = (f32(1.0) - t) if flip else t
            pts.append(t)
            if a * f32(n) == f32(m):
                exact = float(a) * n
                up += int(exact < m)
                down += int(exact > m)
    return pts, up, down


def _windows(n, half=24):
    """the texels of three windows of a strip: both ends and the middle"""
    return sorted(set(list(range(min(n, half))) + list(range(max(n // 2 - half, 0), min(n // 2 + half, n))) + list(range(max(n - half, 0), n))))


def points(W, H):
    """(uv [n, 2] f32, census) of the battery of one size; census counts the points of each class"""
    key = ("uv", W, H)
    if key in _cache:
        return _cache[key]
    strip = max(W, H) > 1024
    cx, cy = _exact_centres(W, False), _exact_centres(H, True)
    uv = [(u, v) for v, _ in cy for u, _ in cx]
    exact = _frozen(np.array([ey and ex for _, ey in cy for _, ex in cx], bool))
    _cache[("exact", W, H)] = exact
    census = dict(centres=len(uv), exact=int(exact.sum()))
    xs = _windows(2 * W + 1) if strip else range(2 * W + 1)
    ys = _windows(2 * H + 1) if strip else range(2 * H + 1)
    grid = [(f32(k / (2 * W)), f32(1.0 - j / (2 * H))) for j in ys for k in xs]
    census["grid"] = len(grid)
    special = [(u, v) for v in SPECIAL for u in SPECIAL]
    census["special"] = len(special)
    ku = _windows(W + 1, 12) if strip else range(W + 1)
    kv = _windows(H + 1, 12) if strip else range(H + 1)
    pu, census["u up"], census["u down"] = _crossing(W, False, ku)
    pv, census["v up"], census["v down"] = _crossing(H, True, kv)
    cross = [(u, f32(0.37)) for u in pu] + [(f32(0.61), v) for v in pv] + [(pu[i % len(pu)], pv[i % len(pv)]) for i in range(max(len(pu), len(pv)))]
    census["crossing"] = len(cross)
    out = _frozen(np.array(uv + grid + special + cross, f32).reshape(-1, 2))
    census["points"] = len(out)
    _cache[key] = (out, census)
    return _cache[key]


def exact_centres(W, H):
    """[W H] bool: which of the first W H points (the texel centres, row-major) have gx and gy exactly integral"""
    points(W, H)
    return _cache[("exact", W, H)]


def image(W, H, C):
    """A random image [H, W, C] in -1 .. 1 with a few exact zeros of both signs"""
    key = ("image", W, H, C)
    if key not in _cache:
        rng = np.random.default_rng(1000 * W + 10 * H + C)
        img = rng.uniform(-1.0, 1.0, (H, W, C)).astype(f32)
        flat = img.reshape(-1)
        flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = f32(0.0)
        flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = f32(-0.0)
        _cache[key] = _frozen(img)
    return _cache[key]


def masked(W, H, C, name):
    """(image [H, W, C] f32, valid [H, W] uint8 or None) of one mask battery"""
    key = ("masked", W, H, C, name)
    if key in _cache:
        return _cache[key]
    img = image(W, H, C)
    y, x = np.mgrid[0:H, 0:W]
    if name == "none":
        valid = None
    elif name == "all":
        valid = np.ones((H, W), np.uint8)
    elif name == "checker":
        valid = ((x + y) % 2 == 0).astype(np.uint8)
    elif name.startswith("parity"):
        valid = ((y % 2 == int(name[6])) & (x % 2 == int(name[7]))).astype(np.uint8)
    elif name == "all invalid":
        valid = np.zeros((H, W), np.uint8)
    elif name == "poison":
        valid = ((x + y) % 2 == 1).astype(np.uint8)
        img = img.copy()
        bad = valid == 0
        img[bad] = np.where(((x + 2 * y) % 3 == 0)[bad][:, None], f32(np.nan), np.where(((x + y) % 4 == 0)[bad][:, None], f32(np.inf), f32(-np.inf)))
    elif name == "spoiled":
        valid = np.ones((H, W), np.uint8) * 255                      # any non-zero byte is valid
        img = img.copy()
        img[H // 2, W // 2] = f32(np.nan)
        img[(H // 2 + 1) % H, (W // 3 + 2) % W, 0] = f32(np.inf)
    else:
        raise KeyError(name)
    _cache[key] = (_frozen(img), None if valid is None else _frozen(valid))
    return _cache[key]


def spoiled_texels(W, H):
    """the texels the 'spoiled' battery made non-finite: [(y, x)]"""
    return [(H // 2, W // 2), ((H // 2 + 1) % H, (W // 3 + 2) % W)]


NORMAL_KINDS = ("unit", "unit", "unnormalised", "unit", "+0", "unnormalised", "-0", "mixed 0", "NaN", "inf", "huge", "unit")


def normals(n, seed=7):
    """[n, 3] f32 normals, the kinds of NORMAL_KINDS in turn: unit, unnormalised (lengths 1e-3 .. 1e3), all-zero of both zero signs and
    mixed, and the non-finite ones (a NaN component, an infinite one, a length that overflows)"""
    key = ("normals", n, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        d = rng.standard_normal((n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        N = d.astype(f32)
        kind = np.arange(n) % len(NORMAL_KINDS)
        for k, name in enumerate(NORMAL_KINDS):
            at = kind == k
            if name == "unnormalised":
                N[at] = (d[at] * 10.0 ** rng.uniform(-3, 3, (int(at.sum()), 1))).astype(f32)
            elif name == "+0":
                N[at] = f32(0.0)
            elif name == "-0":
                N[at] = f32(-0.0)
            elif name == "mixed 0":
                N[at] = np.array([-0.0, 0.0, -0.0], f32)
            elif name == "NaN":
                N[at, 1] = f32(np.nan)
            elif name == "inf":
                N[at, 0] = f32(np.inf)
            elif name == "huge":
                N[at] = (d[at] * 1e30).astype(f32)
        _cache[key] = _frozen(N)
    return _cache[key]


def clean_normals(n):
    """which of normals(n) are finite with a finite, non-zero length in f32"""
    name = np.array(NORMAL_KINDS)[np.arange(n) % len(NORMAL_KINDS)]
    return np.isin(name, ("unit", "unnormalised"))


FORMS = (3, 27, "sh")                    # lightmap_sample at 3 and at 27 channels, lightmap_sh_sample


def inputs(W, H, form, mask):
    """(image, valid, uv, normals or None) of one battery"""
    img, valid = masked(W, H, 3 if form == 3 else 27, mask)
    uv, _ = points(W, H)
    return img, valid, uv, normals(len(uv)) if form == "sh" else None


def reference(W, H, form, flags, mask):
    """(out, weight) of the definition on one battery, computed once"""
    key = ("reference", W, H, form, flags, mask)
    if key not in _cache:
        img, valid, uv, nrm = inputs(W, H, form, mask)
        got = lightmap_sh_sample(img, uv, nrm, valid, flags) if form == "sh" else lightmap_sample(img, uv, valid, flags)
        _cache[key] = tuple(_frozen(a) for a in got)
    return _cache[key]


# ---------------------------------------------------------------- the float64 restatement
def f64_lookup(img, uv, valid, nearest, nrm=None):
    """lightmap_sample (nrm None) or lightmap_sh_sample restated in float64: the tap indices and the fractions f are the definitions'
    (f32: they are the data the sums are made of), everything from the weights on is float64 with no particular order.  Returns
    (out [n, C or 3], weight [n], scale [n, 1 or 3]): scale is what the bounds multiply — max |t| over the finite valid texels for
    the plain form, sum_taps w sum_k |b_k r_k| / sw per colour channel for the SH form."""
    img = np.asarray(img, f32)
    H, W = img.shape[:2]
    img = img.reshape(H, W, -1)
    uv = np.asarray(uv, f32).reshape(-1, 2)
    ok = np.ones((H, W), bool) if valid is None else np.asarray(valid) != 0
    u, v = uv[:, 0], uv[:, 1]
    n = len(uv)
    with np.errstate(all="ignore"):
        if nearest:
            x = np.where(np.isnan(u), 0, np.minimum(np.trunc(np.fmin(np.fmax(u, f32(0)), f32(0.999)) * f32(W)).astype(np.int64), W - 1))
            y = np.where(np.isnan(v), 0, np.minimum(np.trunc((f32(1) - np.fmin(np.fmax(v, f32(0)), f32(0.999))) * f32(H)).astype(np.int64), H - 1))
            taps = [(y, x, np.ones(n))]
        else:
            ix, wx = _lml_axis(u, W)
            iy, wy = _lml_axis(f32(1.0) - v, H)
            fx, fy = wx[1].astype(np.float64), wy[1].astype(np.float64)
            wx, wy = (1.0 - fx, fx), (1.0 - fy, fy)
            taps = [(iy[dy], ix[dx], wx[dx] * wy[dy]) for dy in (0, 1) for dx in (0, 1)]
        if nrm is not None:
            N = np.asarray(nrm, f32).astype(np.float64)
            covered = (N != 0).any(axis=1)
            x, y, z = (N / np.sqrt((N * N).sum(axis=1))[:, None]).T
            b = np.stack([np.ones(n), y, z, x, x * y, y * z, 3.0 * z * z - 1.0, x * z, x * x - y * y], axis=1)
        C = 3 if nrm is not None else img.shape[2]
        acc, sw, mass = np.zeros((n, C)), np.zeros(n), np.zeros((n, 3))
        for yi, xi, w in taps:
            take = (w > 0) & ok[yi, xi]
            t = np.where(take[:, None], img[yi, xi].astype(np.float64), 0.0)
            w = np.where(take, w, 0.0)
            if nrm is not None:
                r = t.reshape(n, 9, 3) * PV_K.astype(np.float64)[None, :, None]
                mass += w[:, None] * np.abs(b[:, :, None] * r).sum(axis=1)
                t = (b[:, :, None] * r).sum(axis=1)
            acc += w[:, None] * t
            sw += w
        out = np.where((sw > 0)[:, None], acc / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
        if nrm is not None:
            out = np.where(covered[:, None], out, 0.0)
            sw = np.where(covered, sw, 0.0)
            scale = np.where((sw > 0)[:, None], mass / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
        else:
            finite = np.where(np.isfinite(img) & ok[..., None], np.abs(img), 0.0)
            scale = np.full((n, 1), float(finite.max()))
    return out, sw, scale


# ---------------------------------------------------------------- the end-to-end scene
CUBE_AT = (0.2, 1.6, -0.3)


def cube_scene():
    """The cube in the Cornell box of the point-table tests (tests/test_gpu_lightmap_sh.py cube_bake): (scene, cube, its index)"""
    if "scene" not in _cache:
        xf = cgmath.mul(cgmath.from_translation(CUBE_AT), cgmath.from_angle_y(25.0), cgmath.from_scale(0.8))
        cube = StaticMesh(fb.cube_mesh(), Lambertian(albedo=(0.7, 0.7, 0.7)), [None] * 5, xf)
        cam = Camera(screen_width=32, screen_height=32, aa_sample_count=16, path_depth=6, max_trace_dist=100.0, gamma=2.0)
        walls = scenes.cornell_walls()
        _cache["scene"] = (Scene(cam, walls + [cube]), cube, len(walls))
    return _cache["scene"]


def camera_rays(size=64, eye=(2.2, 4.2, 2.8), spread=0.8):
    """A size x size table of pinhole rays from `eye` at the cube, pixel centres, row-major: (origins, dirs) [size^2, 3] f32.  The cube
    fills most of the frame (three of its faces show); the rest hits the walls or leaves through the open front."""
    key = ("rays", size, eye, spread)
    if key not in _cache:
        eye64 = np.array(eye, np.float64)
        view = np.array(CUBE_AT, np.float64) - eye64
        view /= np.linalg.norm(view)
        right = np.cross(view, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        up = np.cross(right, view)
        x, y = np.meshgrid(np.arange(size) + 0.5, np.arange(size) + 0.5)
        d = view + spread * ((x / size - 0.5)[..., None] * right + (0.5 - y / size)[..., None] * up)
        o = np.broadcast_to(eye64, d.shape)
        _cache[key] = (_frozen(np.ascontiguousarray(o.reshape(-1, 3), f32)), _frozen(np.ascontiguousarray(d.reshape(-1, 3), f32)))
    return _cache[key]
