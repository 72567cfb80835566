"""Lightmap mips on the GPU: mi_lightmap_mips, mi_lightmap_sample_lod, mi_lightmap_sh_sample_lod and their _device forms against the numpy
definitions lightmap_mips, lightmap_sample_lod and lightmap_sh_sample_lod, BIT FOR BIT, on the batteries of tests/mips_batteries.py
(which tests/test_lightmap_mips_host.py shows to notice one-token mutants of the definitions), the fused pyramid against the
one-level-per-launch form, and the cube's baked lightmap shaded through its mip chain end to end.

Bit-equality is derived as in tests/test_gpu_lightmap_lookup.py: no fused multiply-add, every operation one of + - * /, sqrtf, floorf,
fminf, fmaxf, a comparison or an exact conversion, in a fixed order per texel and per point on both sides; nothing is summed across
lanes, and a child of the pyramid is weighed the same way whether the kernel reads it from LDS or from global memory."""
import os

import numpy as np
import pytest

from cs397raytracingsp22_amd import (Context, abi, lightmap_mip_layout, lightmap_mips, lightmap_sample_lod, lightmap_sh_sample,
                                     lightmap_sh_sample_lod)

import lookup_batteries as lb
import mips_batteries as mb
from mips_batteries import CHANNELS, FORMS, LOD_MASKS, LOD_SIZES, MASKS, SIZES, bits, f32

pytestmark = pytest.mark.gpu

SEED = 5
KNOB = "MI_RT_LMM_LEVELS_PER_LAUNCH"


def on_device(a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda:0"))


def assert_chain(got, want, what, parts=(0, 1, 2)):
    """(mips, valids, coverage) per level against the definition's, bit for bit; level 0 is the input on both sides"""
    for p in parts:
        assert len(got[p]) == len(want[p]), what
        for l, (g, w) in enumerate(zip(got[p], want[p])):
            assert g.shape == w.shape, (what, p, l)
            assert np.array_equal(bits(g), bits(w)) if p != 1 else np.array_equal(g != 0, w != 0), (what, p, l)


def device_mips(ctx, img, valid, levels=0, want_valid=True, want_coverage=True, stream=None, sync=True):
    """The _device form on torch buffers with one guard texel behind each output: the three per-level lists (None for a plane that was
    not asked for) — or, with sync False, the tensors, still in flight"""
    import torch
    dev = torch.device("cuda:0")
    H, W, C = img.shape
    layout = lightmap_mip_layout(W, H, levels)
    total = sum(w * h for w, h, _ in layout[1:])
    t_img = on_device(img)
    t_valid = None if valid is None else on_device(valid)
    mips = torch.full((total + 1, C), -7.0, dtype=torch.float32, device=dev)
    mv = torch.full((total + 1,), 77, dtype=torch.uint8, device=dev)
    cov = torch.full((total + 1,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    ctx.lightmap_mips_device(W, H, C, t_img.data_ptr(), len(layout), mips.data_ptr(), mv.data_ptr() if want_valid else None,
                             cov.data_ptr() if want_coverage else None, None if t_valid is None else t_valid.data_ptr(),
                             stream.cuda_stream if stream is not None else None)
    if not sync:
        return mips, mv, cov, (t_img, t_valid)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(dev)
    return split(img, valid, layout, mips.cpu().numpy(), mv.cpu().numpy() if want_valid else None, cov.cpu().numpy() if want_coverage else None,
                 (mv.cpu().numpy(), cov.cpu().numpy()))


def split(img, valid, layout, mips, mv, cov, raw):
    total = sum(w * h for w, h, _ in layout[1:])
    H, W, C = img.shape
    assert (mips[total] == -7.0).all() and ((raw[0][total:] == 77).all() and (raw[1][total:] == -7.0).all())          # not one texel past the last level
    if mv is None:
        assert (raw[0] == 77).all()                                                                                    # a plane not asked for is not touched
    if cov is None:
        assert (raw[1] == -7.0).all()
    ok = np.ones((H, W), np.uint8) if valid is None else valid

    def levels(flat, first, tail=()):
        return None if flat is None else [first] + [flat[o:o + w * h].reshape((h, w) + tail) for w, h, o in layout[1:]]
    return levels(mips, img, (C,)), levels(mv, ok), levels(cov, np.where(ok != 0, f32(1.0), f32(0.0)))


# ---------------------------------------------------------------- the pyramid: every battery, both entries
@pytest.mark.parametrize("W,H", SIZES)
def test_host_form_has_the_helpers_bits(gpu_ctx, W, H):
    for C_ in CHANNELS:
        for name in MASKS:
            img, valid = mb.masked(W, H, C_, name)
            assert_chain(gpu_ctx.lightmap_mips(img, valid), mb.reference(W, H, C_, name), (W, H, C_, name))
    img, valid = mb.masked(W, H, 27, "charts")
    got = gpu_ctx.lightmap_mips(img, valid, want_valid=False, want_coverage=False)                 # out_valid and out_coverage NULL
    assert got[1] is None and got[2] is None
    assert_chain(got, mb.reference(W, H, 27, "charts"), (W, H, "no planes"), parts=(0,))
    for levels in sorted({1, 2, max(len(got[0]) - 1, 1)}):
        if levels <= len(got[0]):
            assert_chain(gpu_ctx.lightmap_mips(img, valid, levels), tuple(p[:levels] for p in mb.reference(W, H, 27, "charts")), (W, H, levels))
    if len(got[0]) > 1:
        assert gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("W,H", SIZES)
def test_device_form_has_the_helpers_bits(gpu_ctx, W, H):
    for C_ in CHANNELS:
        for name in MASKS:
            img, valid = mb.masked(W, H, C_, name)
            assert_chain(device_mips(gpu_ctx, img, valid), mb.reference(W, H, C_, name), (W, H, C_, name))
    img, valid = mb.masked(W, H, 3, "random20")
    want = mb.reference(W, H, 3, "random20")
    got = device_mips(gpu_ctx, img, valid, want_valid=False, want_coverage=False)                  # the coverage planes in the context's buffer
    assert got[1] is None and got[2] is None
    assert_chain(got, want, (W, H, "no planes"), parts=(0,))
    assert_chain(device_mips(gpu_ctx, img, valid, want_coverage=False), want, (W, H, "no coverage"), parts=(0, 1))


@pytest.mark.parametrize("W,H", ((130, 67), (33, 45)))
def test_one_level_per_launch_gives_the_same_bytes(gpu_ctx, W, H):
    """A context created with the levels-per-launch knob at 1 (the unfused form) against the default, fused one"""
    before = os.environ.get(KNOB)
    os.environ[KNOB] = "1"
    try:
        unfused = Context(0)
    finally:
        if before is None:
            del os.environ[KNOB]
        else:
            os.environ[KNOB] = before
    try:
        for C_ in CHANNELS:
            for name in ("random70", "charts", "null"):
                img, valid = mb.masked(W, H, C_, name)
                a, b = gpu_ctx.lightmap_mips(img, valid), unfused.lightmap_mips(img, valid)
                assert_chain(b, a, (W, H, C_, name))
                assert_chain(b, mb.reference(W, H, C_, name), (W, H, C_, name))
                assert_chain(device_mips(unfused, img, valid, want_coverage=False), a, (W, H, C_, name, "device"), parts=(0, 1))
    finally:
        unfused.close()


# ---------------------------------------------------------------- the trilinear lookups: every battery, both entries
def host_lod(ctx, form, chain, valids, uv, lod, nrm):
    return ctx.lightmap_sh_sample_lod(chain, uv, nrm, lod, valids) if form == "sh" else ctx.lightmap_sample_lod(chain, uv, lod, valids)


def device_lod(ctx, form, chain, valids, uv, lod, nrm, stream=None, want_weight=True, sync=True, levels=None):
    """The _device form on torch buffers with one guard row behind each output: (out, weight) as numpy — or, with sync False, the
    tensors, still in flight"""
    import torch
    dev = torch.device("cuda:0")
    H, W, C_in = chain[0].shape
    L = len(chain) if levels is None else levels
    n = len(uv)
    C = 3 if form == "sh" else C_in
    t_img = on_device(chain[0])
    t_mips = on_device(mb.pack(chain, (C_in,))) if len(chain) > 1 else None
    t_valid = None if valids is None or valids[0] is None else on_device(valids[0])
    t_mv = on_device(mb.pack(valids)) if valids is not None and len(chain) > 1 else None
    t_uv, t_lod = on_device(uv), on_device(lod)
    t_n = on_device(nrm) if form == "sh" else None
    out = torch.full((n + 1, C), -7.0, dtype=torch.float32, device=dev)
    weight = torch.full((n + 1,), -7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize(dev)
    s = stream.cuda_stream if stream is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()                                        # noqa: E731
    if form == "sh":
        ctx.lightmap_sh_sample_lod_device(W, H, t_img.data_ptr(), L, ptr(t_mips), n, t_uv.data_ptr(), t_n.data_ptr(), t_lod.data_ptr(),
                                          out.data_ptr(), weight.data_ptr() if want_weight else None, ptr(t_valid), ptr(t_mv), 0, s)
    else:
        ctx.lightmap_sample_lod_device(W, H, C, t_img.data_ptr(), L, ptr(t_mips), n, t_uv.data_ptr(), t_lod.data_ptr(), out.data_ptr(),
                                       weight.data_ptr() if want_weight else None, ptr(t_valid), ptr(t_mv), 0, s)
    if not sync:
        return out, weight, (t_img, t_mips, t_valid, t_mv, t_uv, t_lod, t_n)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize(dev)
    o, w = out.cpu().numpy(), weight.cpu().numpy()
    assert (o[n] == -7.0).all() and w[n] == -7.0                              # not one lane past n
    return o[:n], w[:n]


def assert_bits(got, want, what):
    assert np.array_equal(bits(got[0]), bits(want[0])), what
    assert np.array_equal(bits(got[1]), bits(want[1])), what


@pytest.mark.parametrize("W,H", LOD_SIZES)
def test_lod_host_forms_have_the_helpers_bits(gpu_ctx, W, H):
    for form in FORMS:
        for name in LOD_MASKS:
            chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, name)
            assert_bits(host_lod(gpu_ctx, form, chain, valids, uv, lod, nrm), mb.lod_reference(W, H, form, name), (W, H, form, name))
    assert gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("W,H", LOD_SIZES)
def test_lod_device_forms_have_the_helpers_bits(gpu_ctx, W, H):
    for form in FORMS:
        for name in LOD_MASKS:
            chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, name)
            assert_bits(device_lod(gpu_ctx, form, chain, valids, uv, lod, nrm), mb.lod_reference(W, H, form, name), (W, H, form, name))
    assert gpu_ctx.last_kernel_ms() > 0.0


@pytest.mark.parametrize("n", lb.COUNTS)
def test_point_counts_around_a_block(gpu_ctx, n):
    """1, 255, 256 and 257 points: a prefix of the battery gives a prefix of the results, through both entries; no weight asked for"""
    import torch
    W, H = 33, 45
    for form in FORMS:
        chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, "random70")
        want = tuple(a[:n] for a in mb.lod_reference(W, H, form, "random70"))
        nn = None if nrm is None else nrm[:n]
        assert_bits(host_lod(gpu_ctx, form, chain, valids, uv[:n], lod[:n], nn), want, (form, n))
        assert_bits(device_lod(gpu_ctx, form, chain, valids, uv[:n], lod[:n], nn), want, (form, n))
        out, weight, keep = device_lod(gpu_ctx, form, chain, valids, uv[:n], lod[:n], nn, want_weight=False, sync=False)
        torch.cuda.synchronize()
        del keep
        assert np.array_equal(bits(out.cpu().numpy()[:n]), bits(want[0])) and (weight.cpu().numpy() == -7.0).all()
        # a shorter chain of the same buffers: the levels are a prefix, lod is clamped to them
        for levels in (1, 3):
            short = (lightmap_sh_sample_lod(chain[:levels], uv[:n], nn, lod[:n], valids[:levels]) if form == "sh"
                     else lightmap_sample_lod(chain[:levels], uv[:n], lod[:n], valids[:levels]))
            assert_bits(device_lod(gpu_ctx, form, chain, valids, uv[:n], lod[:n], nn, levels=levels), short, (form, n, levels))


# ---------------------------------------------------------------- refusals, and nothing to do
def test_refusals_launch_nothing(gpu_ctx):
    lib = abi.load()
    h = gpu_ctx._h
    W, H, n = 8, 8, 16
    img, valid = np.array(mb.image(W, H, 27)), np.ones((H, W), np.uint8)
    chain, valids, _ = lightmap_mips(img, valid)
    mips, mv = np.ascontiguousarray(mb.pack(chain, (27,))), np.ascontiguousarray(mb.pack(valids))
    uv, lod, nrm = np.array(lb.points(W, H)[0][:n]), np.linspace(0, 3, n).astype(f32), np.array(lb.normals(n))
    assert len(gpu_ctx.lightmap_mips(img, valid)[0]) == 4                            # a launch, so that there is a time to keep
    ms_before = gpu_ctx.last_kernel_ms()
    made = len(mv)
    o_mips, o_valid, o_cov = np.full((made, 27), -7.0, f32), np.full(made, 77, np.uint8), np.full(made, -7.0, f32)
    out, weight = np.full((n, 27), -7.0, f32), np.full(n, -7.0, f32)

    def pyramid(ctx=h, w=W, hh=H, ch=27, image=img.ctypes.data, v=valid.ctypes.data, levels=0, m=o_mips.ctypes.data, ov=o_valid.ctypes.data,
                oc=o_cov.ctypes.data, device=False):
        rc = (lib.mi_lightmap_mips_device(ctx, w, hh, ch, image, v, levels, m, ov, oc, None) if device
              else lib.mi_lightmap_mips(ctx, w, hh, ch, image, v, levels, m, ov, oc))
        assert rc == abi.MI_OK or len(lib.mi_last_error().decode()) > 10
        return rc

    def sample(ctx=h, w=W, hh=H, ch=27, image=img.ctypes.data, v=valid.ctypes.data, levels=0, m=mips.ctypes.data, vm=mv.ctypes.data, count=n,
               pts=uv.ctypes.data, d=lod.ctypes.data, flags=0, o=out.ctypes.data, ww=weight.ctypes.data, device=False):
        rc = (lib.mi_lightmap_sample_lod_device(ctx, w, hh, ch, image, v, levels, m, vm, count, pts, d, flags, o, ww, None) if device
              else lib.mi_lightmap_sample_lod(ctx, w, hh, ch, image, v, levels, m, vm, count, pts, d, flags, o, ww))
        assert rc == abi.MI_OK or len(lib.mi_last_error().decode()) > 10
        return rc

    def sh_sample(ctx=h, w=W, hh=H, image=img.ctypes.data, v=valid.ctypes.data, levels=0, m=mips.ctypes.data, vm=mv.ctypes.data, count=n,
                  pts=uv.ctypes.data, normals=nrm.ctypes.data, d=lod.ctypes.data, flags=0, o=out.ctypes.data, ww=weight.ctypes.data, device=False):
        rc = (lib.mi_lightmap_sh_sample_lod_device(ctx, w, hh, image, v, levels, m, vm, count, pts, normals, d, flags, o, ww, None) if device
              else lib.mi_lightmap_sh_sample_lod(ctx, w, hh, image, v, levels, m, vm, count, pts, normals, d, flags, o, ww))
        assert rc == abi.MI_OK or len(lib.mi_last_error().decode()) > 10
        return rc

    size = [dict(w=0), dict(hh=0), dict(w=32769), dict(hh=32769), dict(levels=5), dict(levels=17), dict(levels=0xFFFFFFFF)]
    looks = size + [dict(image=None), dict(pts=None), dict(d=None), dict(o=None), dict(ctx=None), dict(m=None), dict(m=None, levels=2),
                    dict(flags=1), dict(flags=2), dict(flags=3), dict(flags=0x80000000)]
    for device in (False, True):          # every refusal comes before a pointer is used: the host arrays stand in for device memory here
        for kw in size + [dict(image=None), dict(m=None), dict(ctx=None), dict(ch=0), dict(ch=1), dict(ch=4), dict(ch=9), dict(ch=28)]:
            assert pyramid(device=device, **kw) == abi.MI_ERR_INVALID, (kw, device)
        for kw in looks + [dict(ch=0), dict(ch=1), dict(ch=4), dict(ch=28)]:
            assert sample(device=device, **kw) == abi.MI_ERR_INVALID, (kw, device)
        for kw in looks + [dict(normals=None)]:
            assert sh_sample(device=device, **kw) == abi.MI_ERR_INVALID, (kw, device)
        # MI_OK and nothing launched: one level, a 1 x 1 image, no point
        assert pyramid(device=device, levels=1) == abi.MI_OK and pyramid(device=device, w=1, hh=1) == abi.MI_OK
        assert sample(device=device, count=0) == abi.MI_OK and sh_sample(device=device, count=0) == abi.MI_OK
    # an output that overlaps an input (the device forms), from either end (every address below does overlap: a call that passed would
    # hand host memory to a kernel)
    rec, msk = H * W * 108, H * W
    for kw, size_ in (("m", made * 108), ("ov", made), ("oc", made * 4)):
        for at in (img.ctypes.data, img.ctypes.data + rec - 4, img.ctypes.data - size_ + 4, valid.ctypes.data + msk - 1):
            assert pyramid(device=True, **{kw: at}) == abi.MI_ERR_INVALID and "overlap" in lib.mi_last_error().decode(), (kw, at)
    for call, inputs in ((sample, (img, valid, mips, mv, uv, lod)), (sh_sample, (img, valid, mips, mv, uv, lod, nrm))):
        for kw, size_ in (("o", n * 12), ("ww", n * 4)):
            for a in inputs:
                for at in (a.ctypes.data, a.ctypes.data + a.nbytes - 1, a.ctypes.data - size_ + 1):
                    assert call(device=True, **{kw: at}) == abi.MI_ERR_INVALID and "overlap" in lib.mi_last_error().decode(), (kw, at)
    assert (o_mips == -7.0).all() and (o_valid == 77).all() and (o_cov == -7.0).all() and (out == -7.0).all() and (weight == -7.0).all()
    assert gpu_ctx.last_kernel_ms() == ms_before                                     # nothing was launched
    # the optional ones may be NULL; one level needs no mips
    assert pyramid(v=None, ov=None, oc=None) == abi.MI_OK and (o_mips != -7.0).all() and (o_valid == 77).all() and (o_cov == -7.0).all()
    assert sample(v=None, vm=None, ww=None) == abi.MI_OK and (out != -7.0).all() and (weight == -7.0).all()
    assert sample(levels=1, m=None, vm=None) == abi.MI_OK and (weight != -7.0).all()
    with pytest.raises(ValueError):                                                  # the Python mirror checks before any call
        gpu_ctx.lightmap_sample_lod(chain, uv, lod, valids, abi.MI_LS_NEAREST)
    with pytest.raises(ValueError):
        gpu_ctx.lightmap_mips(img, valid, 5)
    fresh = Context(0)                                                                # no scene is needed
    try:
        assert_bits(fresh.lightmap_sh_sample_lod(chain, uv, nrm, lod, valids), lightmap_sh_sample_lod(chain, uv, nrm, lod, valids), "fresh")
    finally:
        fresh.close()


# ---------------------------------------------------------------- non-finite input
def test_clean_points_keep_their_bits_beside_non_finite_ones(gpu_ctx):
    """Non-finite uv, lod, normals and texels spoil only the points whose taking-part taps touch them: a point with finite uv, lod and
    normal has, beside the others, the bits it has in a call of its own; with a NaN texel in level 0 (valid) the pyramid's NaN are its
    ancestors', and the points that read none of them keep the bits they have on the clean chain"""
    W, H = 33, 45
    for form in FORMS:
        chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, "charts")                       # NaN and infinities behind the mask
        got = host_lod(gpu_ctx, form, chain, valids, uv, lod, nrm)
        assert_bits(got, mb.lod_reference(W, H, form, "charts"), form)
        keep = np.isfinite(uv).all(axis=1) & np.isfinite(lod)
        if form == "sh":
            keep &= lb.clean_normals(len(uv))
        assert 1000 < keep.sum() < len(uv)
        alone = host_lod(gpu_ctx, form, chain, valids, np.array(uv[keep]), np.array(lod[keep]), None if nrm is None else np.array(nrm[keep]))
        assert np.isfinite(alone[0]).all()
        assert_bits((got[0][keep], got[1][keep]), alone, form)
        # a valid NaN texel: through the pyramid and the lookup
        img, valid = mb.masked(W, H, chain[0].shape[2], "random70")
        y, x = np.argwhere(valid != 0)[200]
        spoiled = img.copy()
        spoiled[y, x] = f32(np.nan)
        bad = gpu_ctx.lightmap_mips(spoiled, valid)
        assert_chain(bad, lightmap_mips(spoiled, valid), (form, "spoiled"))
        clean = mb.reference(W, H, chain[0].shape[2], "random70")
        for l in range(len(clean[0])):
            hit = np.zeros(clean[0][l].shape[:2], bool)
            hit[y >> l, x >> l] = True
            assert np.array_equal(np.isnan(bad[0][l]).any(axis=2), hit) and np.array_equal(bits(bad[0][l][~hit]), bits(clean[0][l][~hit]))
        a = host_lod(gpu_ctx, form, bad[0], bad[1], uv, lod, nrm)
        b = host_lod(gpu_ctx, form, clean[0], clean[1], uv, lod, nrm)
        untouched = np.isfinite(a[0]).all(axis=1)                                                # (a point spoiled by its own normal is no witness)
        assert 10 < (~untouched & np.isfinite(b[0]).all(axis=1)).sum() < len(uv) // 2
        assert_bits((a[0][untouched], a[1][untouched]), (b[0][untouched], b[1][untouched]), form)
        assert np.array_equal(bits(a[1]), bits(b[1]))                                            # the weights do not look at the values


# ---------------------------------------------------------------- two streams
def test_two_streams_give_the_bits_of_two_calls_alone(gpu_ctx):
    import torch
    W, H = 33, 45
    a = mb.lod_inputs(W, H, "sh", "random70")
    b = mb.lod_inputs(W, H, 3, "charts")
    img, valid = mb.masked(130, 67, 27, "random20")
    alone = (device_lod(gpu_ctx, "sh", *a), device_lod(gpu_ctx, 3, *b), device_mips(gpu_ctx, img, valid))
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    first = device_lod(gpu_ctx, "sh", *a, stream=s1, sync=False)
    second = device_lod(gpu_ctx, 3, *b, stream=s2, sync=False)
    third = device_mips(gpu_ctx, img, valid, stream=s1, sync=False)                  # its coverage planes are its own: it may overlap
    s1.synchronize()
    s2.synchronize()
    torch.cuda.synchronize()
    n = len(a[2])
    for got, want in ((first, alone[0]), (second, alone[1])):
        assert_bits((got[0].cpu().numpy()[:n], got[1].cpu().numpy()[:n]), want, "streams")
    layout = lightmap_mip_layout(130, 67)
    mips, mv, cov = (t.cpu().numpy() for t in third[:3])
    assert_chain(split(img, valid, layout, mips, mv, cov, (mv, cov)), alone[2], "streams")
    assert_chain(alone[2], mb.reference(130, 67, 27, "random20"), "alone")
    assert_bits(alone[0], mb.lod_reference(W, H, "sh", "random70"), "alone")


# ---------------------------------------------------------------- end to end
def test_the_cube_shaded_through_its_mip_chain(gpu_ctx):
    """Bake the cube's directional lightmap at 64 x 64 in the Cornell box, finish it, build its mips, and shade the 64 x 64 camera rays'
    hits on the cube: at lod = 0 the bits are those of the existing lightmap_sh_sample path; at lod = 2 those of the helper, and every
    hit that had something to read at lod = 0 still has"""
    from dataclasses import replace
    sc, cube, index = lb.cube_scene()
    cam = replace(sc.camera, screen_width=64, screen_height=64, aa_sample_count=4)
    gpu_ctx.upload(sc.flatten())
    sh = gpu_ctx.bake_lightmap_sh(cam, cube, jitter=True, offset=1e-3, seed=SEED)[0]
    assert sh.shape[:2] == (64, 64)
    p1, n1, _ = gpu_ctx.lightmap_texels(cube, 64, 64, rows=1, offset=1e-3)
    rec, valid = gpu_ctx.lightmap_finish_sh(sh, p1[0], n1[0], levels=1, dilate=2)
    chain, valids, cov = gpu_ctx.lightmap_mips(rec, valid)
    assert_chain((chain, valids, cov), lightmap_mips(rec, valid), "cube")
    assert len(chain) == 7 and 0 < cov[-1][0, 0] < 1
    o, d = lb.camera_rays()
    hits = gpu_ctx.intersect_rays(o, d, resolve=True)
    on_cube = (hits.object == index) & hits.has_uv
    assert on_cube.sum() > 1000
    uv, nrm = hits.uv[on_cube], hits.normal[on_cube]
    base = gpu_ctx.lightmap_sh_sample(rec, uv, nrm, valid)                                 # the existing path
    assert_bits(base, lightmap_sh_sample(rec, uv, nrm, valid), "level 0, the existing path")
    assert_bits(gpu_ctx.lightmap_sh_sample_lod(chain, uv, nrm, 0.0, valids), base, "lod 0")
    far = gpu_ctx.lightmap_sh_sample_lod(chain, uv, nrm, 2.0, valids)
    assert_bits(far, lightmap_sh_sample_lod(chain, uv, nrm, 2.0, valids), "lod 2")
    assert (far[1][base[1] > 0] > 0).all() and (base[1] > 0).sum() > 1000
    assert (far[0] > 0).any() and not np.array_equal(bits(far[0]), bits(base[0]))
