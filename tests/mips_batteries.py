"""Data shared by tests/test_lightmap_mips_host.py and tests/test_gpu_lightmap_mips.py: images and masks aimed at the decision edges of
lightmap_mips (tracing.py), the uv x lod points of lightmap_sample_lod / lightmap_sh_sample_lod, the float64 restatements both are held
to, and the source-text mutants of the definitions.  Nothing here needs a GPU.

Sizes (W x H): 1x1, 2x1, 3x5, 33x45 (two 32-texel tiles per axis), 64x64, 97x31 and 130x67, whose full chain has 9 levels: two fused
launches.  Every size runs at 3 and at 27 channels.
Masks per size: all valid, none given (NULL), random 70 %, random 20 %, one valid texel, none valid, and "charts": rectangular charts with
gutters between them, the gutters holding NaN and infinities (none of it may reach an output).
Images: uniform in -1 .. 1 times 10^uniform(-3, 3), six decades, with a few exact zeros of both signs.
Points of the _lod batteries: lookup_batteries.points(W, H) (every texel centre, the half-texel grid, the special coordinates, the
rounding crossings), thinned to about 6000 by a fixed stride at the larger sizes, crossed with the levels of detail
{-1, 0, 0.25, 0.5, 1, 1.75, L - 1, L + 3, NaN, +inf, the f32 neighbours of 1.0 either side}, L the full chain of the size."""
import numpy as np

from cs397raytracingsp22_amd import lightmap_mip_layout, lightmap_mips, lightmap_sample_lod, lightmap_sh_sample_lod, tracing
from cs397raytracingsp22_amd.tracing import PV_K, _lml_axis_lod, _lml_levels

import finish_batteries as fb
import lookup_batteries as lb
from lookup_batteries import bits, f32  # noqa: F401

SIZES = ((1, 1), (2, 1), (3, 5), (33, 45), (64, 64), (97, 31), (130, 67))                     # (W, H)
CHANNELS = (3, 27)
MASKS = ("all", "null", "random70", "random20", "one", "empty", "charts")
LOD_SIZES = ((1, 1), (2, 1), (3, 5), (33, 45), (64, 64), (130, 67))
LOD_MASKS = ("null", "random70", "charts")
FORMS = lb.FORMS                                                                              # 3, 27, "sh"
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def full_chain(W, H):
    return len(lightmap_mip_layout(W, H))


def image(W, H, C):
    key = ("image", W, H, C)
    if key not in _cache:
        rng = np.random.default_rng(7000 * W + 70 * H + C)
        img = (rng.uniform(-1.0, 1.0, (H, W, C)) * 10.0 ** rng.uniform(-3.0, 3.0, (H, W, C))).astype(f32)
        flat = img.reshape(-1)
        flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = f32(0.0)
        flat[rng.integers(0, flat.size, max(flat.size // 50, 1))] = f32(-0.0)
        _cache[key] = _frozen(img)
    return _cache[key]


def mask(W, H, name):
    """valid [H, W] uint8, or None for the "null" battery"""
    key = ("mask", W, H, name)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(31 * W + H)
    y, x = np.mgrid[0:H, 0:W]
    if name == "null":
        valid = None
    elif name == "all":
        valid = np.full((H, W), 255, np.uint8)                         # any non-zero byte is valid
    elif name.startswith("random"):
        valid = (rng.uniform(0.0, 1.0, (H, W)) < int(name[6:]) / 100.0).astype(np.uint8)
    elif name == "one":
        valid = np.zeros((H, W), np.uint8)
        valid[(2 * H) // 3, W // 3] = 1
    elif name == "empty":
        valid = np.zeros((H, W), np.uint8)
    elif name == "charts":                                             # 11 x 7 charts behind gutters of 3 and 2 texels
        valid = ((x % 14 < 11) & (y % 9 < 7)).astype(np.uint8)
    else:
        raise KeyError(name)
    _cache[key] = None if valid is None else _frozen(valid)
    return _cache[key]


def masked(W, H, C, name):
    """(image [H, W, C] f32, valid [H, W] uint8 or None) of one battery; the gutters of "charts" hold NaN and infinities"""
    key = ("masked", W, H, C, name)
    if key not in _cache:
        img, valid = image(W, H, C), mask(W, H, name)
        if name == "charts":
            y, x = np.mgrid[0:H, 0:W]
            img = img.copy()
            bad = valid == 0
            img[bad] = np.where(((x + 2 * y) % 3 == 0)[bad][:, None], f32(np.nan), np.where(((x + y) % 4 == 0)[bad][:, None], f32(np.inf), f32(-np.inf)))
            _frozen(img)
        _cache[key] = (img, valid)
    return _cache[key]


def reference(W, H, C, name, levels=0):
    """(mips, valids, coverage) of the definition on one battery, computed once"""
    key = ("reference", W, H, C, name, levels)
    if key not in _cache:
        img, valid = masked(W, H, C, name)
        _cache[key] = tuple([_frozen(a) for a in part] for part in lightmap_mips(img, valid, levels))
    return _cache[key]


def pack(chain, tail=()):
    """levels 1 .. of a per-level list as the one tight buffer the C calls read and write"""
    parts = [np.asarray(a).reshape((-1,) + tuple(tail)) for a in chain[1:]]
    return np.concatenate(parts) if parts else np.zeros((0,) + tuple(tail), np.asarray(chain[0]).dtype)


# ---------------------------------------------------------------- the uv x lod points
def lods(L):
    one = f32(1.0)
    return np.array([-1.0, 0.0, 0.25, 0.5, 1.0, 1.75, L - 1, L + 3, np.nan, np.inf, np.nextafter(one, f32(0.0)), np.nextafter(one, f32(2.0))], f32)


def lod_points(W, H):
    """(uv [n, 2], lod [n]) f32: the thinned lookup points crossed with lods(full chain)"""
    key = ("lod points", W, H)
    if key not in _cache:
        uv = lb.points(W, H)[0]
        uv = uv[::max(-(-len(uv) // 6000), 1)]
        d = lods(full_chain(W, H))
        _cache[key] = (_frozen(np.ascontiguousarray(np.repeat(uv, len(d), axis=0))), _frozen(np.ascontiguousarray(np.tile(d, len(uv)))))
    return _cache[key]


def lod_inputs(W, H, form, name):
    """(chain, valid_chain or None, uv, lod, normals or None) of one _lod battery: the full chain of the masked image.  With the "null"
    mask no mask is passed at all."""
    mips, valids, _ = reference(W, H, 3 if form == 3 else 27, name)
    uv, lod = lod_points(W, H)
    return mips, None if name == "null" else valids, uv, lod, lb.normals(len(uv)) if form == "sh" else None


def lod_reference(W, H, form, name):
    key = ("lod reference", W, H, form, name)
    if key not in _cache:
        chain, valids, uv, lod, nrm = lod_inputs(W, H, form, name)
        got = lightmap_sh_sample_lod(chain, uv, nrm, lod, valids) if form == "sh" else lightmap_sample_lod(chain, uv, lod, valids)
        _cache[key] = tuple(_frozen(a) for a in got)
    return _cache[key]


# ---------------------------------------------------------------- the float64 restatements
def footprint_sums(a, l):
    """Sums of a [H, W] or [H, W, C] float64 array over the 2^l x 2^l footprints of level l (ceil halving: the last ones are cut off)"""
    s = 1 << l
    H, W = a.shape[:2]
    Hn, Wn = -(-H // s), -(-W // s)
    pad = np.zeros((Hn * s, Wn * s) + a.shape[2:], np.float64)
    pad[:H, :W] = a
    return pad.reshape((Hn, s, Wn, s) + a.shape[2:]).sum(axis=(1, 3))


def f64_mips(img, valid, l):
    """Level l restated in float64 straight from level 0: (mean over the valid texels of the footprint [Hl, Wl, C], their count [Hl, Wl],
    the mean of |t| over them [Hl, Wl, C])"""
    ok = np.ones(img.shape[:2], bool) if valid is None else np.asarray(valid) != 0
    t = np.where(ok[..., None], img.astype(np.float64), 0.0)
    count = footprint_sums(ok.astype(np.float64), l)
    den = np.maximum(count, 1.0)[..., None]
    return footprint_sums(t, l) / den, count, footprint_sums(np.abs(t), l) / den


def f64_lookup_lod(chain, valids, uv, lod, nrm=None):
    """lightmap_sample_lod (nrm None) or lightmap_sh_sample_lod restated in float64: the levels, the tap indices and the fractions are the
    definitions' (f32: they are the data the sums are made of), everything from the weights on is float64 with no particular order.
    Returns (out, weight, scale) as lookup_batteries.f64_lookup: scale is max |t| over the finite valid texels of all levels for the
    plain form, sum_taps w sum_k |B_k r_k| / sw per colour channel for the SH form, B_k = |b_k| but for the two basis functions that are
    differences, B_6 = 3 z^2 + 1 and B_8 = x^2 + y^2 (the images here span six decades: a large r_6 beside a small b_6 would otherwise
    carry roundings the scale does not see)."""
    L = len(chain)
    H0, W0 = chain[0].shape[:2]
    levels = [np.asarray(a, f32).reshape(a.shape[0], a.shape[1], -1) for a in chain]
    oks = [np.ones(a.shape[:2], bool) if valids is None or valids[l] is None else np.asarray(valids[l]) != 0 for l, a in enumerate(levels)]
    uv = np.asarray(uv, f32).reshape(-1, 2)
    n = len(uv)
    u, v = uv[:, 0], uv[:, 1]
    with np.errstate(all="ignore"):
        lv, wl = _lml_levels(np.asarray(lod, f32), L)
        fl = wl[1].astype(np.float64)
        wl = (1.0 - fl, fl)
        if nrm is not None:
            N = np.asarray(nrm, f32).astype(np.float64)
            covered = (N != 0).any(axis=1)
            x, y, z = (N / np.sqrt((N * N).sum(axis=1))[:, None]).T
            b = np.stack([np.ones(n), y, z, x, x * y, y * z, 3.0 * z * z - 1.0, x * z, x * x - y * y], axis=1)
            # what b_6 and b_8 are made of: their roundings are relative to 3 z^2 + 1 and x^2 + y^2, not to the differences
            babs = np.stack([np.ones(n), y, z, x, x * y, y * z, 3.0 * z * z + 1.0, x * z, x * x + y * y], axis=1)
        C = 3 if nrm is not None else levels[0].shape[2]
        acc, sw, mass = np.zeros((n, C)), np.zeros(n), np.zeros((n, 3))
        for side in (0, 1):
            for l in range(L):
                at = np.nonzero((lv[side] == l) & (wl[side] > 0))[0]
                if len(at) == 0:
                    continue
                H, W = levels[l].shape[:2]
                s = f32(2.0 ** -l)
                ix, wx = _lml_axis_lod(u[at], W0, s, W)
                iy, wy = _lml_axis_lod(f32(1.0) - v[at], H0, s, H)
                fx, fy = wx[1].astype(np.float64), wy[1].astype(np.float64)
                wx, wy = (1.0 - fx, fx), (1.0 - fy, fy)
                for dy in (0, 1):
                    for dx in (0, 1):
                        yi, xi = iy[dy], ix[dx]
                        w = wl[side][at] * wx[dx] * wy[dy]
                        take = (w > 0) & oks[l][yi, xi]
                        t = np.where(take[:, None], levels[l][yi, xi].astype(np.float64), 0.0)
                        w = np.where(take, w, 0.0)
                        if nrm is not None:
                            r = t.reshape(len(at), 9, 3) * PV_K.astype(np.float64)[None, :, None]
                            mass[at] += w[:, None] * np.abs(babs[at][:, :, None] * r).sum(axis=1)
                            t = (b[at][:, :, None] * r).sum(axis=1)
                        acc[at] += w[:, None] * t
                        sw[at] += w
        out = np.where((sw > 0)[:, None], acc / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
        if nrm is not None:
            out = np.where(covered[:, None], out, 0.0)
            sw = np.where(covered, sw, 0.0)
            scale = np.where((sw > 0)[:, None], mass / np.where(sw > 0, sw, 1.0)[:, None], 0.0)
        else:
            top = max(float(np.where(np.isfinite(a) & ok[..., None], np.abs(a), 0.0).max()) for a, ok in zip(levels, oks))
            scale = np.full((n, 1), top)
    return out, sw, scale


# ---------------------------------------------------------------- source-text mutants (finish_batteries.mutant's machinery)
mutant = fb.mutant
MIPS_BLOCKS = (tracing._lmm_extent, tracing._lmm_full, tracing.lightmap_mip_layout, tracing.check_lightmap_mips, tracing._lmm_level)
LOD_BLOCKS = (tracing._lm_covered, tracing._lmm_extent, tracing._lmm_full, tracing.lightmap_mip_layout, tracing.check_lightmap_lookup,
              tracing.check_lightmap_lod, tracing._lml_axis_lod, tracing._lml_levels, tracing._lml_lookup_lod)
MIPS_MUTANTS = {
    "dy and dx swapped": ("for dy, dx in _LMM_CHILDREN:", "for dx, dy in _LMM_CHILDREN:"),
    "c > 0 becomes c >= 0": ("& (c > 0)", "& (c >= 0)"),
    "0.25 dropped": ("sc * f32(0.25)", "sc"),
    "floor halving in place of ceil": ("return (n + (1 << l) - 1) >> l", "return max(n >> l, 1)"),
    "the in-bounds test dropped": ("take = inside & (c > 0)", "take = (c > 0)"),
}
LOD_MUTANTS = {
    "2^-l applied after the - 0.5": ("g = (t * f32(n0)) * s - f32(0.5)", "g = (t * f32(n0) - f32(0.5)) * s"),
    "level weights swapped": ("(f32(1.0) - fl, fl)", "(fl, f32(1.0) - fl)"),
    "fmax(lod, 0) dropped": ("np.fmin(np.fmax(lod, f32(0.0)), f32(L - 1))", "np.fmin(lod, f32(L - 1))"),
}
LAST_LEVEL = ("np.minimum(np.floor(lam).astype(np.int64), max(L - 2, 0))", "np.floor(lam).astype(np.int64)")


def same_chain(got, want):
    """Do two results of lightmap_mips agree in sizes and bits?"""
    for g, w in zip(got, want):
        if len(g) != len(w):
            return False
        for a, b in zip(g, w):
            if a.shape != b.shape or not np.array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b):
                return False
    return True


def mips_differs(wrong, sizes=SIZES):
    """Does the mutant's pyramid differ from the definition's on at least one battery?"""
    for W, H in sizes:
        for C in CHANNELS:
            for name in MASKS:
                img, valid = masked(W, H, C, name)
                if not same_chain(wrong(img, valid), reference(W, H, C, name)):
                    return True
    return False


def lod_differs(wrong, form, sizes=LOD_SIZES):
    """Does the mutant's lookup (values or weights) differ from the definition's on at least one battery?"""
    for W, H in sizes:
        for name in LOD_MASKS:
            chain, valids, uv, lod, nrm = lod_inputs(W, H, form, name)
            got = wrong(chain, uv, nrm, lod, valids) if form == "sh" else wrong(chain, uv, lod, valids)
            want = lod_reference(W, H, form, name)
            if not (np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))):
                return True
    return False
