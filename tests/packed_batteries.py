"""Data shared by tests/test_lightmap_packed_host.py and tests/test_gpu_lightmap_packed.py: f32 inputs aimed at the decision edges of the
two encoders of lightmap_pack (tracing.py), packed words for lightmap_unpack, and the source-text mutants of the encoders.  Nothing here
needs a GPU; the arrays are cached and read-only.

f16 (f16_values, a flat f32 array): all 65536 binary16 patterns decoded; for every pair of adjacent finite f16 values of either sign the
exact midpoint (12 significant bits: an f32) and its two f32 neighbours, where round-to-nearest-even decides; +-65504, 65520 (the first
value that would round to infinity), the f32 neighbours of 65504, +-inf; NaNs of both signs and several payloads; +-0, f32 subnormals,
2^-24 (the smallest f16 subnormal), 2^-25 (its half: a tie to zero) and its neighbours, and the f32 either side of 2^-14 (the
smallest normal).
RGB9E5 (rgb_texels, [n, 3] f32): for every e in 0 .. 31 a largest channel at 511.5 2^(e-24) and its f32 neighbours, in each of the three
channel positions (where ms == 512 bumps the exponent); channel values at (q + 0.5) 2^(e-24) and their neighbours beside a fixed
maximum; (0.5 - 2^-25) 2^(e-24), which rounds up by definition; negatives, -0.0, NaN and +inf in every position; 65408, its neighbours
and 70000; maxima below 2^-16 down to subnormal and zero; log-uniform random texels.
Decode (rgb_words): 2^16 random words and every word with e in {0, 31} and mantissas in {0, 1, 255, 256, 511}.
COUNTS: texel counts of 1, 63, 64, 65 and 257 at both channel counts, so block tails and odd 54-byte records are met."""
import itertools

import numpy as np

from cs397raytracingsp22_amd import abi, lightmap_pack, lightmap_unpack, tracing

import finish_batteries as fb
from lookup_batteries import bits, f32  # noqa: F401

F16, RGB9E5 = abi.MI_LP_F16, abi.MI_LP_RGB9E5
COUNTS = (1, 63, 64, 65, 257)
CHANNELS = (3, 27)
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def _around(x):
    """x and its two f32 neighbours"""
    x = f32(x)
    return [np.nextafter(x, f32(-np.inf)), x, np.nextafter(x, f32(np.inf))]


def from_bits(words):
    return np.array(words, np.uint32).view(f32)


NANS = from_bits([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345, 0x7FA00000, 0xFFFFE000])


def f16_values():
    """the f16 battery: a flat f32 array whose length is a multiple of 27"""
    if "f16" not in _cache:
        every = np.arange(65536, dtype=np.uint16).view(np.float16).astype(f32)
        finite = np.sort(np.unique(every[np.isfinite(every)]).astype(np.float64))            # -65504 .. 65504, one zero
        mid = ((finite[:-1] + finite[1:]) * 0.5).astype(f32)
        assert np.array_equal(mid.astype(np.float64), (finite[:-1] + finite[1:]) * 0.5)      # exact in f32
        mids = np.concatenate([np.nextafter(mid, f32(-np.inf)), mid, np.nextafter(mid, f32(np.inf))])
        edge = [65504.0, -65504.0, 65520.0, -65520.0, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1e-40, 2.0 ** -126, -2.0 ** -126,
                2.0 ** -24, -2.0 ** -24, 1e30, -1e30, 3.4e38]
        for x in (65504.0, 65520.0, 2.0 ** -25, -2.0 ** -25, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, 1.5 * 2.0 ** -24, 2.0 ** -15):
            edge += _around(x)
        flat = np.concatenate([every, mids, np.array(edge, f32), NANS])
        flat = np.concatenate([flat, np.zeros(-len(flat) % 27, f32)])
        _cache["f16"] = _frozen(flat)
    return _cache["f16"]


def rgb_texels():
    """the RGB9E5 battery: [n, 3] f32"""
    if "rgb" not in _cache:
        rows = []

        def placed(m, a, b):
            """the value m in each of the three channel positions, a and b in the other two"""
            rows.extend([(m, a, b), (a, m, b), (a, b, m)])
        for e in range(32):
            s = 2.0 ** (e - 24)
            for m in _around(511.5 * s):                                     # the ms == 512 bump and its two sides
                placed(m, f32(0.25 * s), f32(255.5 * s))
            for m in _around(256.0 * s) + _around(512.0 * s) + _around(511.0 * s):      # the exponent's own boundaries
                placed(m, f32(m) * f32(0.5), f32(0.0))
            placed(f32(300.0 * s), f32(0.49999997) * f32(s), f32(1.5 * s))   # (0.5 - 2^-25) scaled rounds UP: the definition
            placed(f32(300.0 * s), np.nextafter(f32(0.49999997), f32(0)) * f32(s), f32(0.5 * s))
        for e in (0, 1, 15, 16, 24, 31):                                     # every q + 0.5 step beside a maximum that fixes e
            s = 2.0 ** (e - 24)
            for q in range(0, 511):
                for c in _around((q + 0.5) * s):
                    rows.append((f32(511.0 * s), c, f32(q * s)))
        for bad in (-1.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, -1e-30, NANS[3], NANS[4]):
            placed(f32(bad), f32(0.75), f32(3.0))
            placed(f32(bad), f32(bad), f32(1e-3))
            rows.append((bad, bad, bad))
        for top in _around(65408.0) + [f32(70000.0), f32(65504.0), f32(3.4e38)] + _around(65280.0) + _around(32768.0):
            placed(top, f32(1000.0), f32(65407.0))
        for tiny in [2.0 ** -16, 2.0 ** -17, 2.0 ** -20, 2.0 ** -24, 1.5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -126, 1e-40, 1e-45, 0.0] + _around(2.0 ** -25) + _around(2.0 ** -16):
            placed(f32(tiny), f32(tiny) * f32(0.5), f32(0.0))
        rng = np.random.default_rng(95)
        rand = (rng.uniform(0.0, 1.0, (4096, 3)) * 2.0 ** rng.uniform(-28.0, 17.0, (4096, 1)) * 2.0 ** rng.uniform(-9.0, 0.0, (4096, 3))).astype(f32)
        _cache["rgb"] = _frozen(np.concatenate([np.array(rows, f32), rand]))
    return _cache["rgb"]


def rgb_words():
    """the decode battery: uint32 words"""
    if "words" not in _cache:
        rng = np.random.default_rng(59)
        rand = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
        edge = [r | g << 9 | b << 18 | e << 27 for e in (0, 31) for r, g, b in itertools.product((0, 1, 255, 256, 511), repeat=3)]
        _cache["words"] = _frozen(np.concatenate([rand, np.array(edge, np.uint32)]))
    return _cache["words"]


def f16_words(C):
    """every binary16 pattern as uint16 [n, C] (padded with zeros)"""
    every = np.arange(65536, dtype=np.uint16)
    return _frozen(np.concatenate([every, np.zeros(-65536 % C, np.uint16)]).reshape(-1, C))


def counted(n, C):
    """n texels of C channels [n, C] f32 over six decades of both signs with a NaN, an infinity and both zeros among them"""
    key = ("counted", n, C)
    if key not in _cache:
        rng = np.random.default_rng(100 * n + C)
        t = (rng.uniform(-1.0, 1.0, (n, C)) * 10.0 ** rng.uniform(-6.0, 5.0, (n, C))).astype(f32)
        flat = t.reshape(-1)
        flat[::7] = np.abs(flat[::7])
        flat[flat.size // 2] = f32(np.nan)
        flat[flat.size // 3] = f32(np.inf)
        flat[0] = f32(-0.0)
        _cache[key] = _frozen(t)
    return _cache[key]


def pack_batteries():
    """[(name, format, texels [n, C] f32)]: every input of mi_lightmap_pack the tests use"""
    if "pack" not in _cache:
        v = f16_values()
        out = [("f16 values x 3", F16, v.reshape(-1, 3)), ("f16 values x 27", F16, v.reshape(-1, 27)), ("rgb texels", RGB9E5, rgb_texels()),
               ("rgb texels as f16", F16, rgb_texels())]
        for n in COUNTS:
            out += [(f"{n} x 3 f16", F16, counted(n, 3)), (f"{n} x 27 f16", F16, counted(n, 27)), (f"{n} x 3 rgb", RGB9E5, counted(n, 3))]
        _cache["pack"] = out
    return _cache["pack"]


def unpack_batteries():
    """[(name, format, packed)]: every input of mi_lightmap_unpack the tests use"""
    if "unpack" not in _cache:
        out = [("f16 patterns x 3", F16, f16_words(3)), ("f16 patterns x 27", F16, f16_words(27)), ("rgb words", RGB9E5, rgb_words())]
        for n in COUNTS:
            out += [(f"{n} x 3 f16", F16, _frozen(lightmap_pack(counted(n, 3), F16))), (f"{n} x 27 f16", F16, _frozen(lightmap_pack(counted(n, 27), F16))),
                    (f"{n} rgb", RGB9E5, rgb_words()[5 * n:6 * n])]
        _cache["unpack"] = out
    return _cache["unpack"]


def packed_reference(name):
    """lightmap_pack's bits of one pack battery, computed once"""
    key = ("packed", name)
    if key not in _cache:
        _, fmt, x = next(b for b in pack_batteries() if b[0] == name)
        _cache[key] = _frozen(lightmap_pack(x, fmt))
    return _cache[key]


def unpacked_reference(name):
    key = ("unpacked", name)
    if key not in _cache:
        _, fmt, p = next(b for b in unpack_batteries() if b[0] == name)
        _cache[key] = _frozen(lightmap_unpack(p, fmt))
    return _cache[key]


# ---------------------------------------------------------------- source-text mutants of the encoders (finish_batteries.mutant's machinery)
mutant = fb.mutant
PACK_BLOCKS = (tracing._check_packed_format, tracing._pow2_f32)
_TOWARD_ZERO = ("np.where(np.abs(c.astype(np.float16).astype(f32)) > np.abs(c), np.nextafter(c.astype(np.float16), np.float16(0.0)), "
                "c.astype(np.float16)).view(np.uint16)")
PACK_MUTANTS = {
    "rint for floor(x + 0.5)": ("q = np.floor(c * _pow2_f32(24 - e)[..., None] + f32(0.5))", "q = np.rint(c * _pow2_f32(24 - e)[..., None])"),
    "no ms == 512 bump": ("e = ep + (ms == f32(512.0))", "e = ep"),
    "-15 for -16": ("np.maximum(eb, -16)", "np.maximum(eb, -15)"),
    "clamp at 65504 for 65408": ("f32(65408.0)", "f32(65504.0)"),
    "NaN not zeroed": ("np.where(x != x, f32(0.0), np.fmin(", "np.where(x != x, x, np.fmin("),
    "f16 clamp dropped": ("c = np.fmin(np.fmax(x, f32(-65504.0)), f32(65504.0))", "c = x"),
    "truncation for round-to-nearest-even": ("bits = c.astype(np.float16).view(np.uint16)", "bits = " + _TOWARD_ZERO),
    "NaN through the conversion": ("np.where(x != x, np.uint16(0x7E00), bits)", "bits"),
    "negative channels not clamped": ("np.fmax(x, f32(0.0))", "x"),
}


def pack_differs(wrong):
    """the names of the pack batteries on which the mutant's words differ from the definition's"""
    found = []
    with np.errstate(all="ignore"):
        for name, fmt, x in pack_batteries():
            if not np.array_equal(wrong(x, fmt), packed_reference(name)):
                found.append(name)
    return found
