"""The output stage on caller-made buffers: mi_tonemap_device (fb_tonemap_u8, tracing.rs:244-256) and mi_unpermute_device
(fb_unpermute) — HIP through the C ABI against a float64 restatement, the oracle's tonemap_pixel and dist.compact_index.

Tonemap.  A 257 x 3 image (771 pixels: the last 256-thread block has idle lanes) per gamma in {1, 1.8, 2, 2.2, 2.4, 0.5}: special pixels
(values > 1 in one, two and three channels for the saturate-to-white carries, negatives, +-0, denormals, +-inf, NaN in each channel), the two
f32 neighbours of every c at which c^(1/gamma) * 255.9999 crosses an integer (255 crossings), and a dense sweep of [0, 1].  The restatement
does the f32 carries first (tmp[i] - 1 added to the other two channels, in the reference's order), clamps, and raises to 1/gamma (the f32
quotient 1.0f / gamma) in float64: p64.  The kernel's powf may return any f32 within DELTA / 255.9999 of p64; the u8 must be
floor(f32(p * 255.9999f)) for one such p — so away from an integer crossing exactly floor(q64), q64 = f32(p64) * 255.9999f as the reference
multiplies it (one f32 product), and either neighbour within the band.

DELTA is measured, not guessed: the largest |powf32 - pow64| * 255.9999 of the C library's powf (the one the oracle's tonemap_pixel calls)
over these same inputs and gammas is 7.6e-06 (half an ulp of a value in [0.5, 1), times 256: that powf rounds correctly on every input
here), doubled because two libms differ by about as much as each does from the truth: DELTA = 1.53e-05.  A test without a GPU
(test_delta_is_measured_on_the_cpu) re-measures the figure on the host's C library, requires it to be at most DELTA / 2, and ties it to the
oracle: tonemap_pixel's bytes are exactly the ones that powf gives.  At most 1 % of the sweep's values may lie in the band (asserted there
and in the GPU test; the share is printed).
Against orc.tonemap_pixel itself the suite's bar of 1 LSB holds; NaN and negative inputs give exactly 0."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from cs397raytracingsp22_amd import Camera
from cs397raytracingsp22_amd import dist as pdist

GAMMAS = [1.0, 1.8, 2.0, 2.2, 2.4, 0.5]
K32 = np.float32(255.9999)
DELTA = 1.53e-05
W, H = 257, 3
F = np.float32


def special_pixels():
    nan, inf = float("nan"), float("inf")
    den, tiny = 1e-45, 1.1754944e-38
    up = float(np.nextafter(F(1), F(2)))
    P = [(1.5, 0.2, 0.1), (0.2, 1.5, 0.1), (0.1, 0.2, 1.5), (up, 0.5, 0.25), (0.5, 0.25, up),                     # one channel over
         (1.25, 1.5, 0.1), (0.1, 1.25, 1.5), (1.5, 0.1, 1.25), (up, up, 0.0),                                     # two
         (1.25, 1.5, 2.0), (3.0, 3.0, 3.0), (up, up, up), (1.0, 1.0, 1.0), (1.0625, 0.9375, 0.96875), (1e30, 0.0, 0.0), (3e38, 3e38, 3e38),
         (-0.5, 0.3, -1e-30), (-1.0, -2.0, -3e38), (-0.25, 1.5, 0.5), (1.75, -0.5, -1.0),                          # negatives, and carried into
         (0.0, -0.0, 0.0), (-0.0, -0.0, -0.0), (den, -den, 64 * den), (tiny, -tiny, tiny / 2), (den, 1.5, -den),
         (inf, 0.5, 0.25), (0.5, inf, 0.25), (0.5, 0.25, inf), (-inf, 0.5, 0.25), (0.5, -inf, 0.25), (0.5, 0.25, -inf), (inf, -inf, 0.5), (inf, inf, inf),
         (nan, 0.5, 0.25), (0.5, nan, 0.25), (0.5, 0.25, nan), (nan, nan, nan), (nan, 1.5, 0.25), (1.5, nan, 0.25), (inf, nan, -inf), (nan, -1.0, 2.0)]
    return np.array(P, np.float32)


def crossing_neighbours(inv_gamma32):
    """The two f32 neighbours of every c with c^(1/gamma) * 255.9999 == n, n = 1 .. 255."""
    n = np.arange(1, 256, dtype=np.float64)
    c = (n / float(K32)) ** (1.0 / float(inv_gamma32))
    lo = c.astype(np.float32)
    lo = np.where(lo.astype(np.float64) > c, np.nextafter(lo, F(0)), lo).astype(np.float32)
    return np.stack([lo, np.nextafter(lo, F(2))], axis=1).reshape(-1)


def make_image(inv_gamma32):
    sp = special_pixels()
    cr = crossing_neighbours(inv_gamma32)
    assert len(cr) % 3 == 0
    n_sweep = (W * H - len(sp)) * 3 - len(cr)
    sweep = np.linspace(0.0, 1.0, n_sweep).astype(np.float32)
    img = np.concatenate([sp.reshape(-1), cr, sweep]).astype(np.float32).reshape(H, W, 3)
    is_sweep = np.zeros(W * H * 3, bool)
    is_sweep[len(sp) * 3 + len(cr):] = True
    return img, is_sweep.reshape(H, W, 3), len(sp)


def carried(img):
    """tracing.rs:244-251 in f32: every channel above 1 adds its excess to the other two, in channel order."""
    tmp = img.reshape(-1, 3).astype(np.float32)
    fc = tmp.copy()
    with np.errstate(all="ignore"):
        for i in range(3):
            d = tmp[:, i] - F(1.0)
            m = d > 0
            for j in ((i + 1) % 3, (i + 2) % 3):
                fc[m, j] = fc[m, j] + d[m]
    return fc


def clamp01(fc):
    with np.errstate(all="ignore"):
        c = np.where(fc < 0, F(0), fc)
        return np.where(c > 1, F(1), c).astype(np.float32)          # NaN stays NaN, as in f32::clamp


def allowed_u8(c32, inv_gamma32, delta):
    """[lo, hi] of the u8 a conforming kernel may return for the clamped f32 value c32; NaN -> 0."""
    c = c32.astype(np.float64)
    with np.errstate(all="ignore"):
        p64 = np.power(c, float(inv_gamma32))
    dp = delta / float(K32)

    def to_f32(v, up):
        x = v.astype(np.float32)
        x64 = x.astype(np.float64)
        if up:      # smallest f32 >= v
            return np.where(x64 < v, np.nextafter(x, F(np.inf)), x).astype(np.float32)
        return np.where(x64 > v, np.nextafter(x, F(-np.inf)), x).astype(np.float32)
    plo, phi = to_f32(p64 - dp, True), to_f32(p64 + dp, False)
    single = plo > phi                                              # no f32 inside the band: the nearest one
    near = p64.astype(np.float32)
    plo, phi = np.where(single, near, plo), np.where(single, near, phi)

    def quant(p):
        q = (p.astype(np.float32) * K32).astype(np.float32)
        out = np.where(q >= 255.0, 255, np.floor(np.where(q > 0, q, 0))).astype(np.int64)
        return np.where(np.isnan(q), 0, out)
    return quant(plo), quant(phi), quant(near)      # `near`: the f64 power rounded once to f32, then the reference's f32 product and `as u8`


def libm_powf():
    lib = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    lib.powf.argtypes, lib.powf.restype = [C.c_float, C.c_float], C.c_float
    return lib.powf


@pytest.mark.parametrize("gamma", GAMMAS)
def test_delta_is_measured_on_the_cpu(orc, gamma):
    """DELTA on the host, no GPU: the largest |powf32 - pow64| * 255.9999 of the C library's powf over the image's clamped values is at
    most DELTA / 2, the oracle's tonemap_pixel returns exactly the bytes that powf gives (so the figure IS the oracle's), and at most 1 %
    of the sweep lies within DELTA of an integer crossing."""
    inv_g = F(1.0) / F(gamma)
    img, is_sweep, _ = make_image(inv_g)
    c32 = clamp01(carried(img))
    powf = libm_powf()
    flat = c32.reshape(-1)
    ok = ~np.isnan(flat)
    p32 = np.array([powf(float(x), float(inv_g)) for x in flat[ok]], np.float32)
    measured = float(np.max(np.abs(p32.astype(np.float64) - np.power(flat[ok].astype(np.float64), float(inv_g)))) * float(K32))
    lo, hi, _ = allowed_u8(c32, inv_g, DELTA)
    share = float((lo != hi).reshape(-1)[is_sweep.reshape(-1)].mean())
    print(f"gamma {gamma}: libm |powf32 - pow64| * 255.9999 max {measured:.3e} (DELTA {DELTA:.3e}); {share:.4%} of the sweep in the band")
    assert measured <= DELTA / 2
    assert share <= 0.01
    q = (p32 * K32).astype(np.float32)
    mine = np.zeros(flat.shape, np.int64)
    mine[ok] = np.where(q >= 255.0, 255, np.floor(q)).astype(np.int64)
    ref = np.stack([orc.tonemap_pixel(px, gamma) for px in img.reshape(-1, 3)]).astype(np.int64).reshape(-1)
    assert np.array_equal(mine, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", GAMMAS)
def test_tonemap_on_a_made_buffer(gpu_ctx, orc, gamma):
    import torch
    inv_g = F(1.0) / F(gamma)                                       # mi_rt.cpp and the oracle: 1.0f / gamma
    img, is_sweep, n_special = make_image(inv_g)
    dev = torch.device("cuda:0")
    t_img = torch.from_numpy(img).to(dev)
    guard = 64
    t_u8 = torch.full((W * H * 3 + guard,), 0xA5, dtype=torch.uint8, device=dev)
    cam = Camera(screen_width=W, screen_height=H, gamma=gamma)
    torch.cuda.synchronize()
    gpu_ctx.tonemap_device(cam, t_img.data_ptr(), t_u8.data_ptr())
    torch.cuda.synchronize()
    raw = t_u8.cpu().numpy()
    assert np.all(raw[W * H * 3:] == 0xA5)                          # nothing past the last pixel
    got = raw[: W * H * 3].reshape(-1, 3).astype(np.int64)

    fc = carried(img)
    c32 = clamp01(fc)
    lo, hi, exact = allowed_u8(c32, inv_g, DELTA)
    band = lo != hi
    share = float(band.reshape(-1)[is_sweep.reshape(-1)].mean())
    print(f"gamma {gamma}: DELTA {DELTA:.3e}; in the band: {int(band.sum())} values, {share:.4%} of the sweep; special pixels {n_special}")
    assert share <= 0.01
    bad = (got < lo) | (got > hi)
    assert not bad.any(), (gamma, np.argwhere(bad)[:8], got[bad][:8], lo[bad][:8], hi[bad][:8], c32[bad][:8])
    assert np.array_equal(got[~band], exact[~band])                  # away from a crossing: exactly floor(q64)
    # NaN and negative inputs give exactly 0 (a NaN channel never carries; a negative one may be carried INTO)
    assert np.all(got[np.isnan(fc)] == 0) and np.all(got[fc < 0] == 0)
    # the carries saturate toward white
    sp = special_pixels()
    for k, px in enumerate(sp):
        if tuple(px) in ((np.inf, 0.5, 0.25), (3.0, 3.0, 3.0), (np.inf, np.inf, np.inf)):
            assert tuple(got[k]) == (255, 255, 255), (px, got[k])
    assert got[0][0] == 255 and got[0][1] > 0
    # against the oracle's tonemap_pixel: 1 LSB
    ref = np.stack([orc.tonemap_pixel(px, gamma) for px in img.reshape(-1, 3)]).astype(np.int64)
    assert np.max(np.abs(got - ref)) <= 1, int(np.max(np.abs(got - ref)))
    print(f"gamma {gamma}: {int((got != ref).sum())} of {got.size} bytes differ from the oracle by 1")


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("size", [(1, 1), (33, 1), (31, 65), (96, 54)])
def test_unpermute_on_a_made_buffer(gpu_ctx, size, world):
    import torch
    w, h = size
    padded = pdist.tiles_padded(w, h, world)
    n = world * padded * pdist.TILE_PIXELS * 3
    assert n < 1 << 24                                              # every flat index is an exact f32
    dev = torch.device("cuda:0")
    gathered = torch.arange(n, dtype=torch.float32, device=dev)
    guard = 96
    image = torch.full((h * w * 3 + guard,), -7.0, dtype=torch.float32, device=dev)
    cam = Camera(screen_width=w, screen_height=h)
    torch.cuda.synchronize()
    gpu_ctx.unpermute_device(cam, world, gathered.data_ptr(), image.data_ptr())
    torch.cuda.synchronize()
    raw = image.cpu().numpy()
    assert np.all(raw[h * w * 3:] == -7.0)
    rank, idx = pdist.compact_index(w, h, world)
    want = ((rank * padded * pdist.TILE_PIXELS + idx) * 3)[:, :, None] + np.arange(3)[None, None, :]
    assert np.array_equal(raw[: h * w * 3].reshape(h, w, 3).astype(np.int64), want)
    # more ranks than tiles (the grid's padding columns hold no pixel either): some rank's buffer is never read
    _, _, total = pdist.tile_grid(w, h, world)
    assert len(np.unique(rank)) <= min(world, total)
    if (w, h) == (1, 1):
        assert len(np.unique(rank)) == 1
