"""Packed lightmaps on the host: the numpy definitions lightmap_pack, lightmap_unpack, lightmap_sample_packed and lightmap_sh_sample_packed
(tracing.py) against the facts the formats' construction gives, the validator against the C side's refusals, the C++ mirror
(host/tracing.hpp Scene::pack_lightmap / unpack_lightmap, a stand-alone program) against the helpers on the batteries' bytes, and the
batteries of tests/packed_batteries.py shown to notice one-token mutants of the two encoders.  No GPU.

The bounds asserted here are derived, not measured.  f16: round-to-nearest-even to 11 significant bits is off by at most half a unit in
the last place, 2^-11 |x| for a normal result, and by at most half a subnormal step, 2^-25, below 2^-14.  RGB9E5: a channel is rounded to
a multiple of 2^(e-24) by floor(. + 0.5), off by at most half a step, 2^(e-25); where e > 0 the largest channel m is at least
255.5 2^(e-24) before a bump and maps to 256 .. 511 steps, so half a step is at most m / 511."""
import os
import subprocess

import numpy as np
import pytest

from cs397raytracingsp22_amd import (abi, check_lightmap_packed, lightmap_pack, lightmap_sample, lightmap_sample_lod,
                                     lightmap_sample_packed, lightmap_sh_sample, lightmap_sh_sample_lod, lightmap_sh_sample_packed,
                                     lightmap_unpack)

import lookup_batteries as lb
import mips_batteries as mb
import packed_batteries as pb
from packed_batteries import F16, RGB9E5, bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the formats' own facts
def test_every_finite_f16_pattern_round_trips():
    words = np.arange(65536, dtype=np.uint16).reshape(-1, 1).repeat(3, axis=1)
    x = lightmap_unpack(words, F16)
    back = lightmap_pack(x, F16)
    finite = np.isfinite(x)
    assert finite.sum() == 3 * 63488 and np.array_equal(back[finite], words[finite])             # subnormals and both zeros included
    assert (back[np.isnan(x)] == 0x7E00).all()                                                    # one NaN, by a select
    assert set(back[np.isinf(x)].tolist()) == {0x7BFF, 0xFBFF}                                    # no infinity is ever written


def test_f16_is_round_to_nearest_even_saturating():
    x = pb.f16_values()
    got = lightmap_unpack(lightmap_pack(x.reshape(-1, 3), F16), F16).reshape(-1).astype(np.float64)
    finite = np.isfinite(x)
    c = np.clip(x[finite].astype(np.float64), -65504.0, 65504.0)
    err = np.abs(got[finite] - c)
    assert (err <= np.where(np.abs(c) >= 2.0 ** -14, np.abs(c) * 2.0 ** -11, 2.0 ** -25)).all()
    assert np.isnan(got[np.isnan(x)]).all() and np.isfinite(got[~np.isnan(x)]).all()
    assert np.array_equal(np.signbit(got[finite]), np.signbit(x[finite]))                         # the sign of zero is kept
    one = lambda v: int(lightmap_pack(np.array([v, 0, 0], f32), F16)[0])                          # noqa: E731
    assert [one(v) for v in (65504.0, 65520.0, np.inf, 1e30, -65520.0, -np.inf)] == [0x7BFF] * 4 + [0xFBFF] * 2
    assert [one(v) for v in (2.0 ** -24, 2.0 ** -25, np.nextafter(f32(2.0 ** -25), f32(1)), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24)] == [1, 0, 1, 2, 2]
    assert one(-0.0) == 0x8000 and one(-1e-45) == 0x8000 and one(np.nextafter(f32(2.0 ** -14), f32(0))) == 0x0400
    assert all(one(v) == 0x7E00 for v in pb.NANS)


def test_rgb9e5_round_trip_ranges_and_error_bounds():
    words = pb.rgb_words()
    x = lightmap_unpack(words, RGB9E5)
    assert np.array_equal(bits(lightmap_unpack(lightmap_pack(x, RGB9E5), RGB9E5)), bits(x))       # decode(encode(decode(w))) == decode(w)
    assert x.max() == f32(65408.0) == lightmap_unpack(np.array([(31 << 27) | 511], np.uint32), RGB9E5)[0, 0]
    t = pb.rgb_texels()
    w = lightmap_pack(t, RGB9E5)
    e = (w >> np.uint32(27)).astype(np.int64)
    got = lightmap_unpack(w, RGB9E5).astype(np.float64)
    with np.errstate(invalid="ignore"):
        c = np.where(np.isnan(t), 0.0, np.clip(t.astype(np.float64), 0.0, 65408.0))
    err = np.abs(got - c)
    half = 2.0 ** (e - 25)[:, None]                                                              # half a step of the texel's exponent
    m = c.max(axis=1)[:, None]
    rand = slice(len(t) - 4096, len(t))                                                          # the log-uniform random texels
    assert (err[rand] <= half[rand]).all() and (err[rand][e[rand] > 0] <= (m[rand] / 511.0)[e[rand] > 0]).all()
    # Aimed at the rounding itself the battery goes beyond half a step, as the definition says it must: y + 0.5f is rounded to f32 before
    # the floor.  For y >= 0.5 the sum stays in y's binade (exact) or crosses into the next with frac(y) >= 0.5 already; for y < 0.5 the
    # sum lies in [0.5, 1), where an ulp is 2^-24, so y in [0.5 - 2^-25, 0.5) rounds up to 1: the excess is at most 2^-25 of a step.
    assert (err <= half * (1.0 + 2.0 ** -24)).all() and (err > half).any()
    assert (err[e > 0] <= (m / 511.0 * (1.0 + 2.0 ** -24))[e > 0]).all() and (e > 0).sum() > 1000 and (e == 0).sum() > 100
    m = m[:, 0]
    assert set(e.tolist()) == set(range(32))
    # the largest channel holds 256 .. 511 steps wherever the exponent is not pinned at 0
    q = np.stack([(w >> np.uint32(9 * k)) & np.uint32(511) for k in range(3)], axis=1).max(axis=1)
    assert (q[e > 0] >= 256).all()


def test_rgb9e5_decision_edges_by_hand():
    one = lambda r, g, b: int(lightmap_pack(np.array([r, g, b], f32), RGB9E5))                     # noqa: E731
    word = lambda r, g, b, e: r | g << 9 | b << 18 | e << 27                                      # noqa: E731
    for e in range(31):
        s = 2.0 ** (e - 24)
        assert one(511.5 * s, 0, 0) == word(256, 0, 0, e + 1)                                     # ms == 512: the exponent is bumped
        assert one(np.nextafter(f32(511.5 * s), f32(0)), 0, 0) == word(511, 0, 0, e)
        assert one(0, 300 * s, f32(0.49999997) * f32(s)) == word(0, 300, 1, e)                    # 0.5 - 2^-25 rounds UP: the definition
        assert one(0, 300 * s, np.nextafter(f32(0.49999997), f32(0)) * f32(s)) == word(0, 300, 0, e)
    assert one(65408.0, 70000.0, np.inf) == word(511, 511, 511, 31) and one(1.0, 0.5, 0.25) == word(256, 128, 64, 16)
    assert one(-1.0, -0.0, np.nan) == 0 and one(np.nan, np.nan, np.nan) == 0 and one(-np.inf, 1e-45, 2.0 ** -26) == 0
    below = np.nextafter(f32(2.0 ** -25), f32(0))                                                 # 0.5 - 2^-25 steps: up, by the same rule
    assert one(2.0 ** -25, 0, 0) == 1 and one(below, 0, 0) == 1 and one(np.nextafter(below, f32(0)), 0, 0) == 0   # below 2^-16 e stays 0
    assert one(0, 2.0 ** -16, 0) == word(0, 256, 0, 0) and one(0, 0, 2.0 ** -15) == word(0, 0, 256, 1)


def test_shapes_and_types():
    x = pb.counted(65, 27)
    p = lightmap_pack(x.reshape(5, 13, 27), F16)
    assert p.dtype == np.uint16 and p.shape == (5, 13, 27) and lightmap_unpack(p, F16).shape == (5, 13, 27)
    assert np.array_equal(lightmap_pack(x.reshape(5, 13, 9, 3), F16).reshape(-1), p.reshape(-1))  # [.., 9, 3] records: the same bytes
    w = lightmap_pack(pb.counted(63, 3).reshape(7, 9, 3), RGB9E5)
    assert w.dtype == np.uint32 and w.shape == (7, 9) and lightmap_unpack(w, RGB9E5).shape == (7, 9, 3)
    for bad in (lambda: lightmap_pack(x, RGB9E5), lambda: lightmap_pack(x, 0), lambda: lightmap_pack(x, 3), lambda: lightmap_pack(x[:, :4], F16),
                lambda: lightmap_unpack(p.astype(np.float16), F16), lambda: lightmap_unpack(w.astype(np.int64), RGB9E5),
                lambda: lightmap_unpack(p, 0), lambda: lightmap_unpack(p[..., :5], F16)):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- the validator
def test_check_refuses_what_the_c_side_refuses():
    W, H = 5, 3
    img3, img27 = lb.image(W, H, 3), lb.image(W, H, 27)
    h3, h27, w3 = lightmap_pack(img3, F16), lightmap_pack(img27, F16), lightmap_pack(img3, RGB9E5)
    uv = lb.points(W, H)[0][:7]
    nrm = lb.normals(7)
    chain = [lightmap_pack(a, F16) for a in mb.reference(W, H, 27, "random70")[0]]
    packed, checked = check_lightmap_packed(h27, F16, uv, None, None, abi.MI_LS_NEAREST, nrm, sh=True)
    assert len(packed) == 1 and packed[0].dtype == np.uint16 and checked[3] == abi.MI_LS_NEAREST
    packed, checked = check_lightmap_packed(chain, F16, uv, 1.5)
    assert len(packed) == len(chain) == len(checked[0]) and checked[3].shape == (7,)
    check_lightmap_packed([w3], RGB9E5, uv, None, [np.ones((H, W))])
    refusals = [
        lambda: check_lightmap_packed(h3, 0, uv),                                               # f32 takes the unpacked calls
        lambda: check_lightmap_packed(h3, 3, uv),                                               # an unknown format
        lambda: check_lightmap_packed(h27.view(np.uint32)[..., :1].reshape(H, W), RGB9E5, uv, normals=nrm, sh=True),    # SH is f16 only
        lambda: check_lightmap_packed(h3, F16, uv, normals=nrm, sh=True),                       # the SH form reads 27 channels
        lambda: check_lightmap_packed(h27, F16, uv, sh=True),                                   # ... and normals
        lambda: check_lightmap_packed(w3, F16, uv),                                             # the wrong words for the format
        lambda: check_lightmap_packed(h3, RGB9E5, uv),
        lambda: check_lightmap_packed(chain, F16, uv),                                          # lod None reads level 0 alone
        lambda: check_lightmap_packed(chain[:1], F16, uv, None, [None, None]),
        lambda: check_lightmap_packed(chain, F16, uv, 0.0, None, abi.MI_LS_NEAREST),            # everything the f32 calls refuse
        lambda: check_lightmap_packed(chain + [chain[-1]], F16, uv, 0.0),
        lambda: check_lightmap_packed([chain[0], chain[2]], F16, uv, 0.0),
        lambda: check_lightmap_packed(h3, F16, uv, None, None, 2),
        lambda: check_lightmap_packed(h3, F16, uv[:, :1]),
        lambda: check_lightmap_packed(h3, F16, uv, None, np.ones((H, W + 1))),
        lambda: check_lightmap_packed(h3, F16, uv, np.zeros(6)),
        lambda: check_lightmap_packed([], F16, uv),
        lambda: check_lightmap_packed(h3[:, :, :2], F16, uv),
    ]
    for k, bad in enumerate(refusals):
        with pytest.raises(ValueError):
            bad()
            pytest.fail(f"refusal {k} passed")


# ---------------------------------------------------------------- a packed lookup is the f32 lookup of the unpacked texels
def formats_of(form):
    return (F16, RGB9E5) if form == 3 else (F16,)


@pytest.mark.parametrize("W,H", lb.SMALL)
def test_level_zero_lookups_are_the_f32_lookups_of_the_unpacked_image(W, H):
    for form in lb.FORMS:
        for name in lb.MASKS:
            img, valid, uv, nrm = lb.inputs(W, H, form, name)
            for fmt in formats_of(form):
                with np.errstate(all="ignore"):
                    p = lightmap_pack(img, fmt)
                back = lightmap_unpack(p, fmt)
                for flags in (0, abi.MI_LS_NEAREST):
                    if form == "sh":
                        got, want = lightmap_sh_sample_packed(p, fmt, uv, nrm, None, valid, flags), lightmap_sh_sample(back, uv, nrm, valid, flags)
                    else:
                        got, want = lightmap_sample_packed([p], fmt, uv, None, [valid], flags), lightmap_sample(back, uv, valid, flags)
                    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (form, name, fmt, flags)


@pytest.mark.parametrize("W,H", mb.LOD_SIZES)
def test_lod_lookups_are_the_f32_lookups_of_the_unpacked_chain(W, H):
    for form in mb.FORMS:
        for name in mb.LOD_MASKS:
            chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, name)
            for fmt in formats_of(form):
                with np.errstate(all="ignore"):
                    p = [lightmap_pack(a, fmt) for a in chain]
                back = [lightmap_unpack(a, fmt) for a in p]
                if form == "sh":
                    got, want = lightmap_sh_sample_packed(p, fmt, uv, nrm, lod, valids), lightmap_sh_sample_lod(back, uv, nrm, lod, valids)
                else:
                    got, want = lightmap_sample_packed(p, fmt, uv, lod, valids), lightmap_sample_lod(back, uv, lod, valids)
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (form, name, fmt)


def test_nearest_returns_the_decoded_texel_as_it_stands():
    img = np.array([[[-0.0, 1.0 / 3.0, -70000.0]]], f32)
    out, w = lightmap_sample_packed(lightmap_pack(img, F16), F16, np.array([0.5, 0.5], f32), None, None, abi.MI_LS_NEAREST)
    assert np.array_equal(out.view(np.uint32), np.array([-0.0, np.float16(1.0 / 3.0), -65504.0], f32).view(np.uint32)) and w == 1


# ---------------------------------------------------------------- the C++ mirror, a stand-alone program
@pytest.fixture(scope="module")
def cpp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("packed") / "packed_lightmap_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "packed_lightmap_check.cpp"), "-o", str(exe), "-lz"], check=True)
    return str(exe)


def run_cpp(exe, tmp_path, mode, fmt, channels, data, dtype):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(data).tofile(src)
    r = subprocess.run([exe, mode, str(fmt), str(channels), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return np.fromfile(dst, dtype)


def test_the_cpp_mirror_has_the_helpers_bits(cpp, tmp_path):
    for name, fmt, x in pb.pack_batteries():
        got = run_cpp(cpp, tmp_path, "pack", fmt, x.shape[-1], x, np.uint16 if fmt == F16 else np.uint32)
        assert np.array_equal(got, pb.packed_reference(name).reshape(-1)), name
    for name, fmt, p in pb.unpack_batteries():
        ch = 3 if fmt == RGB9E5 else p.shape[-1]
        got = run_cpp(cpp, tmp_path, "unpack", fmt, ch, p, f32)
        assert np.array_equal(bits(got), bits(pb.unpacked_reference(name).reshape(-1))), name
    src = tmp_path / "in.bin"
    np.zeros(27, f32).tofile(src)
    for args in (("pack", "0", "3"), ("pack", "3", "3"), ("pack", "2", "27"), ("pack", "1", "4"), ("unpack", "2", "27"), ("pack", "1", "5")):
        r = subprocess.run([cpp, *args, str(src), str(tmp_path / "none.bin")], capture_output=True, text=True)
        assert r.returncode == 1 and "mi_rt" in r.stderr, args


# ---------------------------------------------------------------- mutants
def test_the_mutant_machinery_changes_nothing():
    same = ("np.maximum(eb, -16)",) * 2
    copy = pb.mutant(lightmap_pack, pb.PACK_BLOCKS, *same)
    assert copy is not lightmap_pack and pb.pack_differs(copy) == []


@pytest.mark.parametrize("name", sorted(pb.PACK_MUTANTS))
def test_batteries_notice_encoder_mutants(name):
    found = pb.pack_differs(pb.mutant(lightmap_pack, pb.PACK_BLOCKS, *pb.PACK_MUTANTS[name]))
    assert found, name
    if "f16" in name or "conversion" in name or "truncation" in name:
        assert "f16 values x 3" in found and "f16 values x 27" in found
    else:
        assert "rgb texels" in found
