"""Data shared by tests/test_lightmap_bc6h_host.py and tests/test_gpu_lightmap_bc6h.py: images and masks aimed at the decision edges of
lightmap_bc6h_encode (tracing.py), blocks for lightmap_bc6h_decode, the big-integer restatement of the encoder both are held to, and the
source-text mutants of the definition.  Nothing here needs a GPU; the arrays are cached and read-only.

Sizes (W x H): 1x1, 4x4, 3x5, 5x4, 8x8, 33x45, 64x64 and 4100x4, which makes 1025 blocks in a row.
Images: the 4 x 4 blocks of an image cycle through eight kinds: random HDR values 2^-20 .. 6e4 per texel and channel; a constant colour;
two colours in a random pattern; a ramp whose green falls while red rises (negatively correlated channels); a smooth ramp of one hue
(what a lightmap mostly holds); random values within one octave; an exact decode of random endpoints, which must survive re-encoding; and four colours on a square in binary16 bits, whose two diagonals
are equally long (the farthest pair's tie rule).
"128x8 flat starts" holds constant and nearly constant blocks at both ends of the range, where the unquantised fields lie 96 and 95 apart.
One more image, 12x4, holds three blocks on which a least-squares round proposes other endpoints of exactly equal error.
Masks: "null" (none passed), "sparse" (the blocks cycle through one texel that takes part, two, none, all and a random half) and the
"charts" of mips_batteries.  The "poison" image holds NaN, +-inf, negatives, -0.0 and values above 65504 both as texels that take part
and behind valid == 0."""
import numpy as np

from cs397raytracingsp22_amd import (lightmap_bc6h_chain, lightmap_bc6h_decode, lightmap_bc6h_encode, lightmap_sample, lightmap_sample_lod,
                                     tracing)

import finish_batteries as fb
import lookup_batteries as lb
import mips_batteries as mb
from lookup_batteries import bits, f32  # noqa: F401

SIZES = ((1, 1), (4, 4), (3, 5), (5, 4), (8, 8), (33, 45), (64, 64), (4100, 4))                # (W, H)
MASKS = ("null", "sparse", "charts")
ROUNDS = (0, 2, 4)
W16 = (0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64)
POISON = np.array([np.nan, np.inf, -np.inf, -1.0, -0.0, 1e9, 65504.0, 65520.0, -np.nan, 70000.0, 3.4e38, -1e-30], np.float32)
# Three blocks (binary16 bits, [16][3] each, found by search) on which a least-squares round proposes other endpoints of EQUAL error: the
# strict-improvement rule keeps the old ones
EQUAL_ERROR_BLOCKS = [[24471, 28919, 2672, 24415, 29029, 2546, 24475, 28941, 2533, 24563, 28940, 2615, 24542, 28868, 2521, 24421, 28920,
    2475, 24436, 29031, 2521, 24397, 28964, 2523, 24566, 29027, 2651, 24454, 29034, 2532, 24473, 28895, 2568, 24391, 28879, 2636, 24557,
    29005, 2508, 24452, 28968, 2473, 24525, 28945, 2516, 24561, 28904, 2495], [7696, 11581, 19465, 7717, 11462, 19513, 7754, 11445,
    19540, 7636, 11566, 19596, 7631, 11424, 19453, 7691, 11580, 19611, 7640, 11520, 19459, 7635, 11498, 19565, 7700, 11457, 19507, 7706,
    11448, 19461, 7788, 11513, 19614, 7756, 11530, 19615, 7662, 11430, 19433, 7780, 11438, 19609, 7654, 11509, 19600, 7718, 11516,
    19438], [14196, 29168, 1477, 14074, 29105, 1431, 14166, 29059, 1511, 14127, 29110, 1602, 14118, 29202, 1594, 14222, 29104, 1584,
    14181, 29161, 1468, 14114, 29016, 1507, 14142, 29159, 1541, 14229, 29214, 1551, 14129, 29097, 1423, 14131, 29184, 1567, 14238,
    29139, 1496, 14228, 29027, 1573, 14230, 29034, 1589, 14232, 29051, 1579]]
_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def block_grid(W, H):
    """(block index [H, W], texel-in-block index [H, W], blocks per row, block rows)"""
    bw, bh = (W + 3) >> 2, (H + 3) >> 2
    y, x = np.mgrid[0:H, 0:W]
    return (y >> 2) * bw + (x >> 2), (y & 3) * 4 + (x & 3), bw, bh


def exact_blocks(n, seed):
    """n random blocks of the one mode whose indices include 0 and 15 and whose fields lie in 1 .. 1022: uint8 [n, 1, 16]"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 16), np.uint8)
    for b in range(n):
        f = rng.integers(1, 1023, 6)
        idx = rng.integers(0, 16, 16)
        idx[rng.integers(1, 8)] = 15
        idx[rng.integers(8, 16)] = 0
        idx[0] &= 7
        out[b] = make_block(f, idx)
    return out.reshape(n, 1, 16)


def make_block(fields, idx, mode=3):
    """the 16 bytes of a block from its six fields (rw gw bw rx gx bx), sixteen indices (texel 0's below 8) and low five bits"""
    v = int(mode)
    for k, q in enumerate(fields):
        v |= int(q) << (5 + 10 * k)
    v |= int(idx[0]) << 65
    for t in range(1, 16):
        v |= int(idx[t]) << (64 + 4 * t)
    return np.frombuffer(v.to_bytes(16, "little"), np.uint8)


def image(W, H):
    key = ("image", W, H)
    if key not in _cache:
        rng = np.random.default_rng(6000 * W + 60 * H)
        blk, tex, bw, bh = block_grid(W, H)
        nb = bw * bh
        kinds = [(rng.uniform(0.5, 1.0, (nb, 16, 3)) * 2.0 ** rng.uniform(-20.0, 15.87, (nb, 16, 3)))]                       # random HDR
        kinds.append(np.repeat(rng.uniform(0.0, 1.0, (nb, 1, 3)) * 2.0 ** rng.uniform(-12.0, 12.0, (nb, 1, 1)), 16, axis=1))  # constant
        two = rng.uniform(0.0, 4.0, (nb, 2, 3))
        kinds.append(two[np.arange(nb)[:, None], rng.integers(0, 2, (nb, 16))])                                             # two colours
        t = (np.arange(16) / 15.0)[None, :, None]
        lo, hi = rng.uniform(0.01, 1.0, (nb, 1, 1)), rng.uniform(1.0, 30.0, (nb, 1, 1))
        kinds.append(np.concatenate([lo + (hi - lo) * t, hi - (hi - lo) * t, np.full((nb, 16, 1), 0.5) + 0.0 * t], axis=2))    # r up, g down
        hue = rng.uniform(0.2, 1.0, (nb, 1, 3))
        kinds.append(hue * (lo + (hi - lo) * ((np.arange(16) % 4 + np.arange(16) // 4) / 6.0)[None, :, None]))              # a smooth ramp
        kinds.append(rng.uniform(1.0, 2.0, (nb, 16, 3)) * 2.0 ** rng.integers(-8, 8, (nb, 1, 1)))                           # one octave
        kinds.append(lightmap_bc6h_decode(exact_blocks(nb, W + H).reshape(nb, 1, 16), 4, 4 * nb).reshape(nb, 16, 3))        # exact decodes
        code = (np.arange(16)[None, :] * 5 + np.arange(nb)[:, None]) % 4                                                     # a square in h: the
        square = rng.integers(2000, 20000, (nb, 1, 3)) + rng.integers(50, 2000, (nb, 1, 1)) * np.stack([code & 1, code >> 1, 0 * code], axis=2)
        kinds.append(square.astype(np.uint16).view(np.float16).astype(np.float64))                                          # diagonals tie
        kind = np.arange(nb) % len(kinds)
        per_block = np.stack(kinds)[kind, np.arange(nb)]                                                                    # [nb, 16, 3]
        _cache[key] = _frozen(np.ascontiguousarray(per_block[blk, tex].astype(f32)))
    return _cache[key]


def mask(W, H, name):
    """valid [H, W] uint8, or None for "null" """
    key = ("mask", W, H, name)
    if key not in _cache:
        if name == "null":
            v = None
        elif name == "charts":
            v = mb.mask(W, H, "charts")
        else:
            rng = np.random.default_rng(17 * W + H)
            blk, tex, _, _ = block_grid(W, H)
            cycle = blk % 5
            first, second = (blk * 7) % 16, (blk * 11 + 5) % 16
            v = np.where(cycle == 0, tex == first, np.where(cycle == 1, (tex == first) | (tex == second), np.where(cycle == 2, False,
                         np.where(cycle == 3, True, rng.uniform(0.0, 1.0, (H, W)) < 0.5)))).astype(np.uint8) * 3
            _frozen(v)
        _cache[key] = v
    return _cache[key]


def poisoned(img, valid, seed):
    """a copy of the image with the POISON values at every seventh texel; and, where a mask is given, behind every texel it excludes"""
    out = img.copy()
    flat = out.reshape(-1, 3)
    rng = np.random.default_rng(seed)
    at = np.arange(seed % 7, len(flat), 7)
    flat[at, rng.integers(0, 3, len(at))] = POISON[rng.integers(0, len(POISON), len(at))]
    if valid is not None:
        gone = np.nonzero(valid.reshape(-1) == 0)[0]
        flat[gone] = POISON[rng.integers(0, len(POISON), (len(gone), 3))]
    return _frozen(out)


def flat_starts():
    """[8, 128, 3] f32: 64 blocks, constant or off by one unit in one texel, whose binary16 bits lie where the unquantised fields are
    96 and 95 apart (h 0 .. 46 and 31697 .. 31743), alone and mixed with ordinary values: the flat start's two fields around c"""
    if "flat" not in _cache:
        rng = np.random.default_rng(77)
        low, high, mid = [0, 5, 16, 17, 20, 23, 24, 29, 30, 35, 46], [31697, 31713, 31714, 31720, 31726, 31727, 31743], [47, 1000, 20000, 31696]
        pools = [low, low, low, high, high, low + high, low + mid, high + mid]
        h = np.array([[pools[b % 8][rng.integers(0, len(pools[b % 8]))] for _ in range(3)] for b in range(64)], np.int64)
        h = np.repeat(h[:, None, :], 16, axis=1)
        odd = np.arange(64) % 4 == 3                                       # every fourth block: one texel one unit up
        h[odd, 5, 1] = np.minimum(h[odd, 5, 1] + 1, 0x7BFF)
        texels = h.astype(np.uint16).view(np.float16).astype(f32).reshape(2, 32, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(8, 128, 3)
        _cache["flat"] = _frozen(np.ascontiguousarray(texels))
    return _cache["flat"]


def encode_batteries():
    """[(name, image [H, W, 3] f32, valid [H, W] uint8 or None)]: every input of mi_lightmap_bc6h_encode the tests use"""
    if "encode" not in _cache:
        out = []
        for W, H in SIZES:
            for name in MASKS:
                out.append((f"{W}x{H} {name}", image(W, H), mask(W, H, name)))
                if (W, H) in ((5, 4), (33, 45)):
                    out.append((f"{W}x{H} {name} poison", poisoned(image(W, H), mask(W, H, name), W + len(name)), mask(W, H, name)))
        h = np.array(EQUAL_ERROR_BLOCKS, np.uint16).reshape(3, 4, 4, 3).transpose(1, 0, 2, 3).reshape(4, 12, 3)
        out.append(("128x8 flat starts", flat_starts(), None))
        out.append(("12x4 equal error", _frozen(np.ascontiguousarray(h.view(np.float16).astype(f32))), None))
        _cache["encode"] = out
    return _cache["encode"]


def battery(name):
    return next(b for b in encode_batteries() if b[0] == name)


def reference(name, rounds):
    """lightmap_bc6h_encode's blocks of one battery, computed once"""
    key = ("blocks", name, rounds)
    if key not in _cache:
        _, img, valid = battery(name)
        _cache[key] = _frozen(lightmap_bc6h_encode(img, valid, rounds))
    return _cache[key]


def decode_batteries():
    """[(name, blocks uint8 [BH, BW, 16], W, H)]: random bytes with every low-five-bit pattern, random blocks of the one mode, the field
    edges 0, 1, 1022, 1023, and the encoder's own output"""
    if "decode" not in _cache:
        rng = np.random.default_rng(66)
        rand = rng.integers(0, 256, (9, 32, 16), dtype=np.uint8)
        rand[..., 0] = (rand[..., 0] & 0xE0) | (np.arange(32, dtype=np.uint8) % 32)[None, :]
        ours = rng.integers(0, 256, (12, 11, 16), dtype=np.uint8)
        ours[..., 0] = (ours[..., 0] & 0xE0) | 3
        edge = np.stack([make_block([a, b, c, c, a, b], (np.arange(16) + s) % 16 & ([7] + [15] * 15))
                         for a in (0, 1, 1022, 1023) for b in (0, 1023, 512) for c in (1, 1022, 1023) for s in (0, 5)]).reshape(8, 9, 16)
        out = [("every mode", _frozen(rand), 125, 33), ("mode 3 random", _frozen(ours), 44, 47), ("field edges", _frozen(edge), 36, 32)]
        for name in ("33x45 charts", "5x4 sparse poison", "1x1 null", "4100x4 null"):
            W, H = battery(name)[1].shape[1], battery(name)[1].shape[0]
            out.append((name, reference(name, 2), W, H))
        _cache["decode"] = out
    return _cache["decode"]


def decoded_reference(name):
    key = ("decoded", name)
    if key not in _cache:
        _, b, W, H = next(d for d in decode_batteries() if d[0] == name)
        _cache[key] = _frozen(lightmap_bc6h_decode(b, W, H))
    return _cache[key]


# ---------------------------------------------------------------- the lookups: chains of mips_batteries, encoded
LOOKUP_SIZES = ((1, 1), (3, 5), (8, 8), (33, 45), (64, 64))
LOOKUP_MASKS = ("null", "random70", "charts")


def chain(W, H, name):
    """(blocks [L], valids [L] or None, decoded levels [L]) of the full mip chain of mips_batteries' image, every level encoded with its
    own mask"""
    key = ("chain", W, H, name)
    if key not in _cache:
        mips, valids, _ = mb.reference(W, H, 3, name)
        with np.errstate(all="ignore"):
            blocks = [_frozen(b) for b in lightmap_bc6h_chain(mips, None if name == "null" else valids, 2)]
        layout = tracing.lightmap_mip_layout(W, H, len(blocks))
        _cache[key] = (blocks, None if name == "null" else valids, [_frozen(lightmap_bc6h_decode(b, wl, hl)) for b, (wl, hl, _) in zip(blocks, layout)])
    return _cache[key]


def lookup_reference(W, H, name, flags):
    """lightmap_sample of decoded level 0 at lookup_batteries' points"""
    key = ("lookup", W, H, name, flags)
    if key not in _cache:
        _, valids, levels = chain(W, H, name)
        uv = lb.points(W, H)[0]
        _cache[key] = tuple(_frozen(a) for a in lightmap_sample(levels[0], uv, None if valids is None else valids[0], flags))
    return _cache[key]


def lod_reference(W, H, name):
    """lightmap_sample_lod of the decoded chain at mips_batteries' uv x lod points"""
    key = ("lod", W, H, name)
    if key not in _cache:
        _, valids, levels = chain(W, H, name)
        uv, lod = mb.lod_points(W, H)
        _cache[key] = tuple(_frozen(a) for a in lightmap_sample_lod(levels, uv, lod, valids))
    return _cache[key]


# ---------------------------------------------------------------- the encoder restated with Python integers, one block at a time
def unq(q):
    return 0 if q == 0 else 0xFFFF if q == 1023 else ((q << 16) + 0x8000) >> 10


UNQ = [unq(q) for q in range(1024)]


def quant_exhaustive(c):
    """the field nearest to c over all 1024, the lower on a tie"""
    c = min(max(c, 0), 65535)
    return min(range(1024), key=lambda q: (abs(UNQ[q] - c), q))


_QUANT = {}


def quant(c):
    c = min(max(c, 0), 65535)
    if c not in _QUANT:
        _QUANT[c] = quant_exhaustive(c)
    return _QUANT[c]


def palette(fields):
    """[16][3] binary16 bits of fields [2][3]"""
    return [[((UNQ[fields[0][k]] * (64 - w) + UNQ[fields[1][k]] * w + 32) >> 6) * 31 >> 6 for k in range(3)] for w in W16]


def assign(target, fields):
    pal = palette(fields)
    idx, err = [], []
    for t in target:
        e = [sum((t[k] - p[k]) ** 2 for k in range(3)) for p in pal]
        idx.append(e.index(min(e)))
        err.append(min(e))
    return idx, err


def half_bits(x):
    """step 1 through float64: the binary16 bits of min(x, 65504) where x > 0, else 0"""
    x = float(x)
    c = min(x, 65504.0) if x > 0.0 else 0.0
    return int(np.float64(c).astype(np.float16).view(np.uint16))


def encode_block(h, part, rounds):
    """one block by the letter of the definition: h [16][3] ints, part [16] bools.  Returns (fields [2][3], indices [16], error), or None
    when nothing takes part"""
    who = [t for t in range(16) if part[t]]
    if not who:
        return None
    best = None
    for i in who:
        for j in who:
            if i <= j:
                d = sum((h[i][k] - h[j][k]) ** 2 for k in range(3))
                if best is None or d > best[0]:
                    best = (d, i, j)
    _, i, j = best
    fields = [[quant(-(-64 * h[t][k] // 31)) for k in range(3)] for t in (i, j)]
    if fields[0] == fields[1]:                                   # a flat start: the two fields around c where the one is far from it
        for k in range(3):
            c = -(-64 * h[i][k] // 31)
            if abs(UNQ[fields[0][k]] - c) > 32:
                fields[0][k], fields[1][k] = (0, 1) if c < 96 else (1022, 1023)
    mean = [sum(h[t][k] for t in who) // len(who) for k in range(3)]
    target = [h[t] if part[t] else mean for t in range(16)]
    idx, e = assign(target, fields)
    err = sum(e[t] for t in who)
    ct = [[-(-64 * h[t][k] // 31) for k in range(3)] for t in range(16)]
    for _ in range(rounds):
        u, v = [64 - W16[idx[t]] for t in range(16)], [W16[idx[t]] for t in range(16)]
        suu, suv, svv = sum(u[t] ** 2 for t in who), sum(u[t] * v[t] for t in who), sum(v[t] ** 2 for t in who)
        det = suu * svv - suv * suv
        cand = [list(fields[0]), list(fields[1])]
        if det != 0:
            for k in range(3):
                suc, svc = sum(u[t] * ct[t][k] for t in who), sum(v[t] * ct[t][k] for t in who)
                na, nb = 64 * (svv * suc - suv * svc), 64 * (suu * svc - suv * suc)
                cand[0][k], cand[1][k] = quant((2 * na + det) // (2 * det)), quant((2 * nb + det) // (2 * det))
        cidx, ce = assign(target, cand)
        cerr = sum(ce[t] for t in who)
        if cerr < err:
            fields, idx, err = cand, cidx, cerr
    if idx[0] >= 8:
        fields, idx = [fields[1], fields[0]], [15 - i for i in idx]
    return fields, idx, err


def encode_restated(img, valid, rounds):
    """lightmap_bc6h_encode restated: uint8 [BH, BW, 16]"""
    H, W = img.shape[:2]
    bw, bh = (W + 3) >> 2, (H + 3) >> 2
    out = np.zeros((bh, bw, 16), np.uint8)
    for by in range(bh):
        for bx in range(bw):
            h, part = [[0, 0, 0] for _ in range(16)], [False] * 16
            for t in range(16):
                x, y = 4 * bx + (t & 3), 4 * by + (t >> 2)
                if x < W and y < H and (valid is None or valid[y, x] != 0):
                    part[t] = True
                    h[t] = [half_bits(img[y, x, k]) for k in range(3)]
            got = encode_block(h, part, rounds)
            out[by, bx] = make_block([0] * 6, [0] * 16) if got is None else make_block(got[0][0] + got[0][1], got[1])
    return out


def block_errors(blocks, img, valid):
    """the error of every block of `blocks` against the image, as the definition counts it: int64 [BH, BW]"""
    H, W = img.shape[:2]
    dec = lightmap_bc6h_decode(blocks, W, H).astype(np.float16).view(np.uint16).astype(np.int64)
    with np.errstate(all="ignore"):
        want = np.where(img > 0, np.minimum(img, f32(65504.0)), f32(0.0)).astype(np.float16).view(np.uint16).astype(np.int64)
    e = ((dec - want) ** 2).sum(axis=-1) * (1 if valid is None else (valid != 0))
    blk, _, bw, bh = block_grid(W, H)
    return _block_sums(e, blk, bw * bh)


def _block_sums(e, blk, nb):
    out = np.zeros(nb, np.int64)
    np.add.at(out, blk.reshape(-1), e.reshape(-1))
    return out


# ---------------------------------------------------------------- source-text mutants of the encoder (finish_batteries.mutant's machinery)
mutant = fb.mutant
ENCODE_BLOCKS = (tracing._bc6h_weights, tracing._bc6h_unq, tracing._bc6h_palette, tracing._bc6h_quant, tracing._bc6h_assign, tracing._bc6h_blocks_of, tracing._bc6h_fit,
                 tracing.check_lightmap_bc6h_image)
ENCODE_MUTANTS = {
    "pair tie to the highest (i, j)": ("d2 * 256 + (255 - (16 * i + j))", "d2 * 256 + (16 * i + j)"),
    "pairs with i > j as well": ("& (i <= j)", "& (i >= j)"),
    "field tie to the higher": ("take = d < bd", "take = d <= bd"),
    "index tie to the highest": ("idx = e.argmin(axis=-1)", "idx = 15 - e[..., ::-1].argmin(axis=-1)"),
    "no anchor swap": ("swap = idx[:, 0] >= 8", "swap = idx[:, 0] >= 16"),
    "anchor at 9": ("swap = idx[:, 0] >= 8", "swap = idx[:, 0] >= 9"),
    "no + 32": ("* w + 32) >> 6", "* w) >> 6"),
    ">> 5 for >> 6": ("return (c * 31) >> 6", "return (c * 31) >> 5"),
    "weight 25 for 26": ("(0, 4, 9, 13, 17, 21, 26, 30,", "(0, 4, 9, 13, 17, 21, 25, 30,"),
    "mask dropped from the error": ("err = (e * part).sum(axis=1)", "err = e.sum(axis=1)"),
    "mask dropped from the sums": ("u, v = (64 - w[idx]) * part, w[idx] * part", "u, v = (64 - w[idx]), w[idx]"),
    "mask dropped from the pair": ("both = part[:, :, None] & part[:, None, :] & (", "both = part[:, :, None] & ("),
    "mean over all sixteen": ("// np.maximum(n, 1)[:, None]", "// 16"),
    "no flat start": ("- c0) > 32)", "- c0) > 48)"),
    "flat start from 31": ("- c0) > 32)", "- c0) > 31)"),
    "flat start at the wrong upper fields": ("np.where(c0 < 96, 0, 1022)", "np.where(c0 < 96, 0, 1021)"),
    "flat start in one channel's view": ("flat = (fields[:, 0] == fields[:, 1]).all(axis=1)", "flat = (fields[:, 0] == fields[:, 1]).any(axis=1)"),
    "kept when not worse": ("better = cerr < err", "better = cerr <= err"),
    "always kept": ("better = cerr < err", "better = cerr < err + (1 << 62)"),
    "floor for ceil in the sums' domain map": ("ct = (64 * h + 30) // 31", "ct = (64 * h) // 31"),
    "round down in the division": ("(2 * na + det) // two", "(2 * na) // two"),
    "NaN through the clamp": ("np.where(img > 0, np.minimum(", "np.where(img == img, np.minimum("),
    "clamp at 65536": ("np.float32(65504.0)", "np.float32(65536.0)"),
}
# An EQUIVALENT mutant: floor for ceil in the START's domain map.  The quantiser decides between neighbouring fields at c = 48 | 49,
# 64 q + 64 | 64 q + 65 and 65487 | 65488.  floor and ceil differ only when 64 h / 31 is no integer, and they straddle a boundary X | X + 1
# only if an integer h lies in (31 X / 64, 31 (X + 1) / 64): (23.25, 23.73), (31 q + 31, 31 q + 31.48) and (31720.27, 31720.75) hold none.
EQUIVALENT_MUTANTS = {
    "floor for ceil in the start's domain map": ("fields = _bc6h_quant((64 * ends + 30) // 31)", "fields = _bc6h_quant((64 * ends) // 31)"),
}


def encode_differs(wrong, rounds=2):
    """the names of the encode batteries on which the mutant's blocks differ from the definition's"""
    found = []
    with np.errstate(all="ignore"):
        for name, img, valid in encode_batteries():
            if not np.array_equal(wrong(img, valid, rounds), reference(name, rounds)):
                found.append(name)
    return found
