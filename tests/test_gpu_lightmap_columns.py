"""The lightmap post-process calls describe their buffers once, as a column list that the host form stages and the device form tests for
overlaps (mi_rt.cpp run_columns).  What such a shared list can get wrong is the layout: an optional buffer that is absent takes no space,
so it shifts every later column of the staging buffer, and one staging buffer serves every family in turn.  So for every family touched
— the four finishes, the eighteen lookups, the mips, pack / unpack, the BC6H coder — the host form and the device form (torch tensors on
the NULL stream, then a synchronise) are called through the raw C ABI with each optional buffer present and absent in turn; both must
give the same BYTES, those of the numpy definition, and write not one byte behind an output.  After every host call the host form of
another family runs and is checked too.

Shapes: the smallest that cross the edges — a 5 x 3 lightmap (odd sizes, a full chain, 2 x 1 BC6H blocks with padded texels), 8 x 8 for
BC6H, 33 x 45 for the mips (two launches: the second reads coverage the first wrote), 3 and 27 channels, 255 / 256 / 257 points (one
block short, exactly, one over) and no points at all.  Inputs: the batteries of the families' own tests."""
import numpy as np
import pytest

from cs397raytracingsp22_amd import (abi, lightmap_bc6h_decode, lightmap_bc6h_encode, lightmap_finish, lightmap_finish_sh,
                                     lightmap_finish_var, lightmap_mips, lightmap_pack, lightmap_sample, lightmap_sample_bc6h,
                                     lightmap_sample_lod, lightmap_sample_packed, lightmap_sh_sample, lightmap_sh_sample_lod,
                                     lightmap_sh_sample_packed, lightmap_unpack)

import bc6h_batteries as bb
import finish_batteries as fb
import lookup_batteries as lb
import mips_batteries as mb
import variance_batteries as vb

pytestmark = pytest.mark.gpu

W, H = 5, 3
MASK = "random70"
COUNTS = (255, 256, 257)
GUARD = 16                    # sentinel bytes behind every output
FILL = 0x77
F16, RGB9E5 = abi.MI_LP_F16, abi.MI_LP_RGB9E5


class Out:
    """An output of `nbytes` bytes: a sentinel-filled buffer with a guard behind it"""
    def __init__(self, want):
        self.want = raw(want)

    def fresh(self):
        return np.full(len(self.want) + GUARD, FILL, np.uint8)


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def both_forms(ctx, name, args):
    """Call mi_lightmap_<name> and mi_lightmap_<name>_device with `args`: numbers as they stand, numpy arrays as inputs, Out as outputs,
    None as NULL.  Asserts that both forms wrote their Outs' wanted bytes and nothing behind them."""
    import torch
    lib = abi.load()
    bufs = [a.fresh() if isinstance(a, Out) else np.ascontiguousarray(a) if isinstance(a, np.ndarray) else a for a in args]
    abi.check(getattr(lib, "mi_lightmap_" + name)(ctx._h, *[b.ctypes.data if isinstance(b, np.ndarray) else b for b in bufs]))
    host = [b for a, b in zip(args, bufs) if isinstance(a, Out)]
    dev = torch.device("cuda:0")
    tens = [torch.from_numpy(a.fresh() if isinstance(a, Out) else np.array(raw(b))).to(dev) if isinstance(b, np.ndarray) else b
            for a, b in zip(args, bufs)]
    assert all(t.data_ptr() % 16 == 0 for t in tens if isinstance(t, torch.Tensor))
    torch.cuda.synchronize()
    abi.check(getattr(lib, "mi_lightmap_" + name + "_device")(ctx._h, *[t.data_ptr() if isinstance(t, torch.Tensor) else t for t in tens], None))
    torch.cuda.synchronize()
    device = [t.cpu().numpy() for a, t in zip(args, tens) if isinstance(a, Out)]
    for k, a in enumerate(o for o in args if isinstance(o, Out)):
        for form, got in (("host", host[k]), ("device", device[k])):
            n = len(a.want)
            wrong = int((got[:n] != a.want).sum())
            assert wrong == 0, (name, form, "output", k, wrong, "bytes differ of", n)
            assert (got[n:] == FILL).all(), (name, form, "output", k, "wrote behind its end")


# ---------------------------------------------------------------- inputs and references, made once
_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def points():
    uv = lb.points(W, H)[0]
    assert len(uv) >= 257
    return uv[:257]


def chain(C):
    """(levels, masks) of the full f32 chain of the 5 x 3 battery image"""
    mips, valids, _ = mb.reference(W, H, C, MASK)
    return mips, valids


def other_family(ctx, mine):
    """The host form of another family, checked against its definition: the staging buffer is one, reused across families"""
    if mine != "pack":
        x = lb.image(W, H, 27)
        want = once("other pack", lambda: lightmap_pack(x, F16))
        assert np.array_equal(ctx.lightmap_pack(x, F16), want), ("pack after", mine)
    else:
        img, valid = mb.masked(W, H, 3, MASK)
        want = once("other sample", lambda: lightmap_sample(img, points(), valid))
        got = ctx.lightmap_sample(img, points(), valid)
        assert np.array_equal(raw(got[0]), raw(want[0])) and np.array_equal(raw(got[1]), raw(want[1])), ("sample after", mine)


# ---------------------------------------------------------------- the finishes
def finish_cases():
    """(name, the arguments behind ctx with Outs for the three outputs) of the four finishes on the 5 x 3 ragged table"""
    _, img, m2, S, P, N, kw = vb.ragged_battery(W, H)
    _, _, _, _, pkw = fb.ragged_battery(W, H)
    sh = np.ascontiguousarray(lb.image(W, H, 27).reshape(H, W, 9, 3) * np.float32(2.0))
    sh = np.where((N == 0).all(axis=-1)[..., None, None], np.float32(0.0), sh)
    y, x = np.mgrid[0:H, 0:W]
    counts = np.ascontiguousarray((2 + (3 * x + y) % 7).astype(np.uint32))
    tail = lambda k: (k["levels"], k["normal_power_log2"], k["sigma_plane"], k["reach"], k["sigma_color"])
    out, valid = once("finish", lambda: lightmap_finish(img, P, N, **pkw))
    yield "finish", (W, H, img, P, N) + tail(pkw) + (pkw["dilate"], Out(out), Out(valid.astype(np.uint8)))
    out, valid = once("finish_sh", lambda: lightmap_finish_sh(sh, P, N, **pkw))
    yield "finish_sh", (W, H, sh, P, N) + tail(pkw) + (pkw["dilate"], Out(out), Out(valid.astype(np.uint8)))
    out, var, valid = once("finish_var", lambda: lightmap_finish_var(img, m2, S, P, N, **kw))
    yield "finish_var", (W, H, img, m2, S, P, N) + tail(kw) + (kw["color_floor"], kw["dilate"], Out(out), Out(var), Out(valid.astype(np.uint8)))
    out, var, valid = once("finish_var_counts", lambda: lightmap_finish_var(img, m2, counts, P, N, **kw))
    yield "finish_var_counts", (W, H, img, m2, counts, P, N) + tail(kw) + (kw["color_floor"], kw["dilate"], Out(out), Out(var),
                                                                        Out(valid.astype(np.uint8)))


def test_the_finishes_with_each_optional_output_present_and_absent(gpu_ctx):
    for name, args in finish_cases():
        optional = [k for k, a in enumerate(args) if isinstance(a, Out)][1:]         # out_var (the variance forms) and out_valid
        for absent in [()] + [(k,) for k in optional] + [tuple(optional)]:
            both_forms(gpu_ctx, name, [None if k in absent else a for k, a in enumerate(args)])
            other_family(gpu_ctx, name)


# ---------------------------------------------------------------- the lookups
def lookup_cases():
    """(name, fmt or None, channels or "sh", chain form?, size) of the eighteen lookups' host / device pairs, both level forms where an
    entry point has both"""
    for C in (3, 27, "sh"):
        sh = C == "sh"
        yield ("sh_sample" if sh else "sample"), None, C, False, (W, H)
        yield ("sh_sample_lod" if sh else "sample_lod"), None, C, True, (W, H)
        for fmt in (F16, RGB9E5) if C == 3 else (F16,):
            for lod in (False, True):
                yield ("sh_sample_packed" if sh else "sample_packed"), fmt, C, lod, (W, H)
    for size in ((W, H), (8, 8)):
        for lod in (False, True):
            yield "sample_bc6h", None, 3, lod, size


CASES = list(lookup_cases())
case_id = lambda c: f"{c[0]}-{c[1]}-{c[2]}-{'lod' if c[3] else 'level0'}-{c[4][0]}x{c[4][1]}"


def stored_levels(case):
    """The levels as the call reads them: f32, packed or blocks; one level for the level-0 form"""
    name, fmt, C, lod, size = case
    if name == "sample_bc6h":
        levels = bb.chain(*size, MASK)[0]
    else:
        levels = chain(27 if C == "sh" else C)[0]
        if fmt is not None:
            levels = once(("packed", C, fmt), lambda: [lightmap_pack(a, fmt) for a in levels])
    return levels if lod else levels[:1]


def lookup_want(name, fmt, C, lod, stored, size, masks, uv, nrm, D):
    """The definition on all 257 points (a lookup is per point: the first n of it are the lookup of the first n points)"""
    def make():
        d = D if lod else None
        if name == "sample_bc6h":
            return lightmap_sample_bc6h(stored, size[0], size[1], uv, d, masks)
        if fmt is not None:
            return lightmap_sh_sample_packed(stored, fmt, uv, nrm, d, masks) if C == "sh" else lightmap_sample_packed(stored, fmt, uv, d, masks)
        if lod:
            return lightmap_sh_sample_lod(stored, uv, nrm, D, masks) if C == "sh" else lightmap_sample_lod(stored, uv, D, masks)
        return lightmap_sh_sample(stored[0], uv, nrm, masks) if C == "sh" else lightmap_sample(stored[0], uv, masks)
    return once(("lookup", name, fmt, C, lod, size, None if masks is None else tuple(m is not None for m in masks) if lod else True), make)


def lookup_args(name, fmt, C, stored, size, v0, mv, n, uv, nrm, D, out, weight):
    """The C argument list behind ctx, as tracing.py Context._lookup assembles it"""
    w, h = size
    has_chain = name not in ("sample", "sh_sample")
    args = (() if fmt is None else (fmt,)) + (w, h) + ((C,) if C != "sh" and name != "sample_bc6h" else ()) + (stored[0], v0)
    if has_chain:
        tail = stored[0].shape[2:]
        mips = mb.pack(stored, tail) if len(stored) > 1 else None
        args += (len(stored), mips, mv)
    args += (n, uv) + ((nrm,) if C == "sh" else ()) + ((D,) if has_chain else ()) + (0, out, weight)
    return list(args)


def lookup_inputs(case):
    name, fmt, C, lod, size = case
    valids = bb.chain(*size, MASK)[1] if name == "sample_bc6h" else chain(27 if C == "sh" else C)[1]
    uv = lb.points(*size)[0][:257] if size != (W, H) else points()
    D = np.ascontiguousarray(np.resize(mb.lods(len(valids)), 257)) if lod else None
    return stored_levels(case), valids, uv, (lb.normals(257) if C == "sh" else None), D


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_lookups_with_each_optional_buffer_present_and_absent(gpu_ctx, case):
    name, fmt, C, lod, size = case
    stored, valids, uv, nrm, D = lookup_inputs(case)
    # (valid, mip_valid, out_weight) present? — all, each absent in turn, none; every count on the first
    present = [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)]
    for k, (has_valid, has_mips, has_weight) in enumerate(present):
        if not has_mips and not (lod and len(stored) > 1) and has_valid and has_weight:
            continue                                                                # no mip_valid to leave out: the first case again
        v0 = np.ascontiguousarray(valids[0], np.uint8) if has_valid else None
        chain_masks = lod and len(stored) > 1 and has_mips
        mv = mb.pack([np.asarray(v, np.uint8) for v in valids]) if chain_masks else None
        if lod:
            masks = None if not has_valid and not chain_masks else [v0] + ([valids[l] for l in range(1, len(stored))] if chain_masks
                                                                           else [None] * (len(stored) - 1))
        else:
            masks = v0
        want, want_w = lookup_want(name, fmt, C, lod, stored, size, masks, uv, nrm, D)
        for n in COUNTS if k == 0 else COUNTS[-1:]:
            args = lookup_args(name, fmt, C, stored, size, v0, mv, n, uv[:n], None if nrm is None else nrm[:n], None if D is None else D[:n],
                               Out(want[:n]), Out(want_w[:n]) if has_weight else None)
            both_forms(gpu_ctx, name, args)
            other_family(gpu_ctx, name)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_no_points_launch_nothing_and_touch_nothing(gpu_ctx, case):
    """n == 0: MI_OK from both forms, the outputs as they were (both_forms' guard starts at byte 0 of an empty want), no timing taken"""
    name, fmt, C, lod, size = case
    stored, valids, uv, nrm, D = lookup_inputs(case)
    other_family(gpu_ctx, name)
    before = gpu_ctx.last_kernel_ms()
    assert before > 0.0
    mv = mb.pack([np.asarray(v, np.uint8) for v in valids]) if lod and len(stored) > 1 else None
    empty = np.zeros((0, 3), np.float32)
    args = lookup_args(name, fmt, C, stored, size, np.ascontiguousarray(valids[0], np.uint8), mv, 0, uv[:1], None if nrm is None else nrm[:1],
                       None if D is None else D[:1], Out(empty), Out(empty))
    both_forms(gpu_ctx, name, args)
    assert gpu_ctx.last_kernel_ms() == before


# ---------------------------------------------------------------- the mips
@pytest.mark.parametrize("size,C", [((W, H), 3), ((W, H), 27), ((33, 45), 3)])
def test_the_mips_with_each_optional_buffer_present_and_absent(gpu_ctx, size, C):
    w, h = size
    img, valid = mb.masked(w, h, C, MASK)
    for has_valid in (True, False):
        mips, valids, cov = mb.reference(w, h, C, MASK) if has_valid else once(("mips", size, C), lambda: lightmap_mips(img, None))
        outs = (Out(mb.pack(mips, (C,))), Out(mb.pack([np.asarray(v, np.uint8) for v in valids])), Out(mb.pack(cov)))
        for has_mask, has_cov in ((True, True), (False, True), (True, False), (False, False)):
            both_forms(gpu_ctx, "mips", [w, h, C, img, valid if has_valid else None, len(mips), outs[0], outs[1] if has_mask else None,
                                         outs[2] if has_cov else None])
            other_family(gpu_ctx, "mips")


# ---------------------------------------------------------------- pack / unpack and the BC6H coder
@pytest.mark.parametrize("fmt,C", [(F16, 3), (F16, 27), (RGB9E5, 3)])
def test_pack_and_unpack(gpu_ctx, fmt, C):
    x = np.ascontiguousarray(mb.image(W, H, C).reshape(-1, C))
    packed = lightmap_pack(x, fmt)
    both_forms(gpu_ctx, "pack", [fmt, C, len(x), x, Out(packed)])
    other_family(gpu_ctx, "pack")
    both_forms(gpu_ctx, "unpack", [fmt, C, len(x), packed, Out(lightmap_unpack(packed, fmt))])
    other_family(gpu_ctx, "pack")


@pytest.mark.parametrize("size", [(W, H), (8, 8)])
def test_the_bc6h_coder_with_the_mask_present_and_absent(gpu_ctx, size):
    w, h = size
    img, valid = bb.image(w, h), bb.mask(w, h, "sparse")
    for v in (valid, None):
        blocks = once(("bc6h", size, v is None), lambda: lightmap_bc6h_encode(img, v, 2))
        both_forms(gpu_ctx, "bc6h_encode", [w, h, img, v, 2, Out(blocks)])
        other_family(gpu_ctx, "bc6h")
        both_forms(gpu_ctx, "bc6h_decode", [w, h, blocks, Out(lightmap_bc6h_decode(blocks, w, h))])
        other_family(gpu_ctx, "bc6h")
