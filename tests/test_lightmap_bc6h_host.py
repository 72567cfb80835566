"""BC6H lightmaps on the host: the numpy definitions lightmap_bc6h_encode, lightmap_bc6h_decode, lightmap_bc6h_layout, lightmap_bc6h_modes
and lightmap_sample_bc6h (tracing.py) against an independent decoder, against the facts the encoder's construction gives (all exact),
against a big-integer restatement of the encoder, the C++ mirror (host/tracing.hpp Scene::encode_lightmap_bc6h / decode_lightmap_bc6h, a
stand-alone program) and render_plan.cpp bc6h_plan against the helpers, and the batteries of tests/bc6h_batteries.py shown to notice
one-token mutants of the encoder.  No GPU.

The bounds asserted here are derived, not measured; the constant-block tests say how."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cs397raytracingsp22_amd import (abi, check_lightmap_bc6h, lightmap_bc6h_chain, lightmap_bc6h_decode, lightmap_bc6h_encode,
                                     lightmap_bc6h_layout, lightmap_bc6h_modes, lightmap_mip_layout, lightmap_sample, lightmap_sample_bc6h,
                                     lightmap_sample_lod, tracing)

import bc6h_batteries as bb
import lookup_batteries as lb
import mips_batteries as mb
from bc6h_batteries import bits, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cs397raytracingsp22_amd", "csrc")


def fields_and_indices(blocks):
    """(fields [n, 2, 3], indices [n, 16], low five bits [n]) of uint8 [..., 16], by Python integers"""
    f, x, m = [], [], []
    for b in np.ascontiguousarray(blocks).reshape(-1, 16):
        v = int.from_bytes(b.tobytes(), "little")
        m.append(v & 31)
        f.append([[(v >> (5 + 10 * (3 * e + k))) & 1023 for k in range(3)] for e in range(2)])
        x.append([(v >> 65) & 7] + [(v >> (64 + 4 * t)) & 15 for t in range(1, 16)])
    return np.array(f), np.array(x), np.array(m)


# ---------------------------------------------------------------- the decoder
def test_the_decoder_agrees_with_an_independent_one():
    """Pillow's bcn decoder (BC6H, unsigned) on random blocks of the one mode with every field below 500, so that every value lies in
    0 .. 1 where Pillow's 8-bit output resolves it: within one 8-bit step after clip(x, 0, 1) * 255"""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(2000):
        idx = rng.integers(0, 16, 16)
        idx[0] &= 7
        block = bb.make_block(rng.integers(0, 500, 6), idx)
        theirs = np.asarray(Image.frombytes("RGB", (4, 4), block.tobytes(), "bcn", 6)).astype(np.float64)
        ours = lightmap_bc6h_decode(block.reshape(1, 1, 16), 4, 4).astype(np.float64)
        worst = max(worst, float(np.abs(np.clip(ours, 0.0, 1.0) * 255.0 - theirs).max()))
    print("largest difference to Pillow, in 8-bit steps:", worst)
    assert worst <= 1.0


def test_the_decoder_by_hand_and_other_modes_are_zeros():
    rand = bb.decode_batteries()[0]
    got = bb.decoded_reference(rand[0])
    _, _, modes = fields_and_indices(rand[1])
    per_block = got[:32, :124].reshape(8, 4, 31, 4, 3).transpose(0, 2, 1, 3, 4).reshape(8 * 31, 48)
    other = (modes.reshape(9, 32)[:8, :31] != 3).reshape(-1)
    assert other.sum() == 8 * 30 and (per_block[other] == 0).all() and (per_block[~other] != 0).any()
    hist = lightmap_bc6h_modes(rand[1])
    assert hist.shape == (32,) and hist.dtype == np.int64 and (hist == 9).all()
    assert lightmap_bc6h_modes(bb.reference("33x45 charts", 2))[3] == 108 and lightmap_bc6h_modes(bb.reference("33x45 charts", 2)).sum() == 108
    # one block by the letter of the format: fields 1023 / 0, every index once
    one = lightmap_bc6h_decode(bb.make_block([1023, 0, 512, 0, 1023, 512], np.arange(16) % 16 & ([7] + [15] * 15)).reshape(1, 1, 16), 4, 4)
    h = one.astype(np.float16).view(np.uint16).reshape(16, 3).astype(np.int64)
    for t in range(16):
        w = bb.W16[t if t else 0]
        assert list(h[t]) == [((0xFFFF * (64 - w) + 32) >> 6) * 31 >> 6, ((0xFFFF * w + 32) >> 6) * 31 >> 6, (32800 * 31) >> 6]
    assert h.max() == 0x7BFF and one.max() == f32(65504.0)
    for bad in (lambda: lightmap_bc6h_decode(np.zeros((1, 1, 16), np.uint8), 5, 4), lambda: lightmap_bc6h_decode(np.zeros((1, 1, 16), np.int8), 4, 4),
                lambda: lightmap_bc6h_decode(np.zeros((1, 1, 16), np.uint8), 0, 4), lambda: lightmap_bc6h_modes(np.zeros((4, 4), np.uint8))):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------- the encoder's properties, all exact
@pytest.mark.parametrize("rounds", bb.ROUNDS)
def test_every_block_is_of_the_one_mode_anchored_and_optimal_in_its_indices(rounds):
    for name, img, valid in bb.encode_batteries():
        blocks = bb.reference(name, rounds)
        H, W = img.shape[:2]
        assert blocks.shape == ((H + 3) >> 2, (W + 3) >> 2, 16) and blocks.dtype == np.uint8
        fields, idx, modes = fields_and_indices(blocks)
        assert (modes == 3).all() and (idx[:, 0] < 8).all(), name
        # for the emitted endpoints every index of a texel that takes part is an exhaustive optimum
        blk, tex, bw, bh = bb.block_grid(W, H)
        with np.errstate(all="ignore"):
            want = np.where(img > 0, np.minimum(img, f32(65504.0)), f32(0.0)).astype(np.float16).view(np.uint16).astype(np.int64)
        pal = tracing._bc6h_palette(fields.astype(np.int64))                                          # [n, 16, 3]
        e = ((want[:, :, None, :] - pal[blk]) ** 2).sum(axis=-1)                                      # [H, W, 16]
        chosen = np.take_along_axis(e, idx[blk, tex][..., None], axis=-1)[..., 0]
        part = np.ones((H, W), bool) if valid is None else valid != 0
        assert (chosen[part] == e.min(axis=-1)[part]).all(), name
        # a block in which nothing takes part is the word 3 and zeros
        took = np.zeros(bw * bh, np.int64)
        np.add.at(took, blk.reshape(-1), part.reshape(-1))
        empty = blocks.reshape(-1, 16)[took == 0]
        assert (empty[:, 0] == 3).all() and (empty[:, 1:] == 0).all(), name
        assert np.isfinite(lightmap_bc6h_decode(blocks, W, H)).all()


def test_texels_that_take_no_part_do_not_move_a_bit():
    rng = np.random.default_rng(3)
    for name, img, valid in bb.encode_batteries():
        if valid is None:
            continue
        other = np.array(img)
        gone = valid == 0
        other[gone] = bb.POISON[rng.integers(0, len(bb.POISON), (int(gone.sum()), 3))]
        again = np.array(img)
        again[gone] = f32(123.0)
        for rounds in (0, 2):
            want = bb.reference(name, rounds)
            with np.errstate(all="ignore"):
                assert np.array_equal(lightmap_bc6h_encode(other, valid, rounds), want) and np.array_equal(lightmap_bc6h_encode(again, valid, rounds), want), name
    # what lies outside the image is not there at all: 5 x 4 and the same image widened to 8 x 4 behind a mask
    img = np.array(bb.image(5, 4))
    wide, mask = np.full((4, 8, 3), np.nan, f32), np.zeros((4, 8), np.uint8)
    wide[:, :5], mask[:, :5] = img, 1
    with np.errstate(all="ignore"):
        assert np.array_equal(lightmap_bc6h_encode(wide, mask), lightmap_bc6h_encode(img))


def test_the_error_never_rises_with_rounds():
    improved = 0
    for name, img, valid in bb.encode_batteries():
        errs = [bb.block_errors(lightmap_bc6h_encode(img, valid, r) if r in (1, 3) else bb.reference(name, r), img, valid) for r in range(5)]
        for a, b in zip(errs, errs[1:]):
            assert (b <= a).all(), name
        improved += int((errs[4] < errs[0]).sum())
    assert improved > 1000                                                                            # the rounds do something


def constant_blocks():
    """(image [4, 4 n, 3], its binary16 bits): n blocks of one colour each, 2^-26 .. 2^16 per channel, and the ends of the range"""
    rng = np.random.default_rng(8)
    colours = np.concatenate([(rng.uniform(0.5, 1.0, (4000, 3)) * 2.0 ** rng.uniform(-26.0, 16.0, (4000, 3))).astype(f32),
                              np.array([[0, 0, 0], [65504, 65504, 65504], [1e9, 6e-8, 0.5], [2.0 ** -24, 2.0 ** -25, 2.0 ** -14]], f32),
                              (np.arange(1, 61, dtype=f32) * f32(2.0 ** -24)).reshape(20, 3)])
    img = np.repeat(np.repeat(colours.reshape(-1, 1, 1, 3), 4, axis=1), 4, axis=2).transpose(1, 0, 2, 3).reshape(4, -1, 3)
    return img, np.minimum(img, f32(65504.0)).astype(np.float16).view(np.uint16).astype(np.int64)


def test_a_constant_block_decodes_within_sixteen_units():
    """Derived.  The unquantised fields are 0, 96, 160, .., 64 q + 32, .., 65440, 65535 and c = ceil(64 h / 31) is the smallest value
    that decodes to h.  Where the nearest field lies within 32 of c both endpoints take it, the decode is floor(31 a / 64) at every
    index, and it is off by at most 32 * 31 / 64 = 15.5 and the floor: 16.  Farther than 32 the nearest can only be between 0 | 96 and
    65440 | 65535, for c in 33 .. 63 and 65473 .. 65502: the flat start gives such a channel both fields, every such channel wants a
    weight between 33 / 96 and 63 / 96 of the way, a span of 31 in c, and the one shared index (values 6 or 7 apart in c) that is best
    in the sum of squares leaves no channel more than two thirds of that span plus a step away: 27 in c, 14 in h."""
    img, h = constant_blocks()
    for rounds in (0, 2):
        got = lightmap_bc6h_decode(lightmap_bc6h_encode(img, None, rounds), img.shape[1], 4).astype(np.float16).view(np.uint16).astype(np.int64)
        print("rounds", rounds, "largest distance:", int(np.abs(got - h).max()))
        assert np.abs(got - h).max() <= 16
        assert np.abs(got - h).max() >= 8                                                             # (and the bound is not idle)


def test_constant_blocks_at_the_ends_of_the_range_by_all_their_channels():
    """every triple of binary16 bits from the two stretches where the fields lie 96 and 95 apart (and a few from between), as constant
    blocks: within 16 units, the same derivation"""
    low, high, mid = np.arange(0, 64, 4) + 1, np.arange(31690, 31744, 4), np.array([100, 9000, 31600])
    for first, second, third in ((low, low, low), (high, high, high), (low, high, mid), (mid, low, low), (high, mid, low)):
        h = np.stack(np.meshgrid(first, second, third, indexing="ij"), axis=-1).reshape(-1, 3)
        img = np.repeat(np.repeat(h.astype(np.uint16).view(np.float16).astype(f32)[None], 4, axis=0), 4, axis=1)
        for rounds in (0, 2):
            got = lightmap_bc6h_decode(lightmap_bc6h_encode(img, None, rounds), img.shape[1], 4).astype(np.float16).view(np.uint16).astype(np.int64)
            assert np.abs(got[0, ::4] - h).max() <= 16, rounds
    img, _ = constant_blocks()
    assert np.array_equal(lightmap_bc6h_encode(img, None, 0)[:, :4000], lightmap_bc6h_encode(img, None, 4)[:, :4000])   # det == 0: nothing to refine


def test_exact_decodes_survive_re_encoding():
    """Decoded blocks whose indices include 0 and 15, sixteen texels taking part, fields in 1 .. 1022: the farthest pair are the two
    endpoints' own colours, c = ceil(64 h / 31) = 64 q + 31 is nearest to 64 q + 32, so the start recovers the fields, the error is 0
    and the strict-improvement rule keeps them"""
    blocks = bb.exact_blocks(3000, 21).reshape(30, 100, 16)
    texels = lightmap_bc6h_decode(blocks, 400, 120)
    for rounds in (0, 2, 4):
        again = lightmap_bc6h_encode(texels, None, rounds)
        assert np.array_equal(bits(lightmap_bc6h_decode(again, 400, 120)), bits(texels)), rounds
        assert (bb.block_errors(again, texels, None) == 0).all()
    f0, _, _ = fields_and_indices(blocks)
    f1, _, _ = fields_and_indices(again)
    same = (f0 == f1).all(axis=(1, 2)) | (f0 == f1[:, ::-1]).all(axis=(1, 2))
    assert same.mean() > 0.99                                                                         # the endpoints themselves come back


def test_the_quantiser_is_the_nearest_field_lower_on_a_tie():
    c = np.arange(-70, 65700, dtype=np.int64)
    got = tracing._bc6h_quant(c)
    want = np.array([bb.quant_exhaustive(int(v)) for v in c[::7]])
    assert np.array_equal(got[::7], want)
    edges = np.array([0, 48, 49, 64, 65, 96, 128, 129, 65440, 65487, 65488, 65535], np.int64)
    assert np.array_equal(tracing._bc6h_quant(edges), [bb.quant_exhaustive(int(v)) for v in edges])
    assert list(tracing._bc6h_quant(np.array([48, 49, 128, 129, 65487, 65488]))) == [0, 1, 1, 2, 1022, 1023]
    assert [int((i * 64 + 7) // 15) for i in range(16)] == list(bb.W16) == list(tracing._bc6h_weights())      # the kernels' closed form
    assert all(bb.W16[15 - i] == 64 - bb.W16[i] for i in range(16))


# ---------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", [b[0] for b in bb.encode_batteries() if not (b[0].startswith("4100") and "null" not in b[0])])
def test_the_big_integer_restatement_has_the_helpers_bytes(name):
    _, img, valid = bb.battery(name)
    for rounds in (bb.ROUNDS if img.shape[0] * img.shape[1] < 2000 else (2,)):
        assert np.array_equal(bb.encode_restated(img, valid, rounds), bb.reference(name, rounds)), (name, rounds)


# ---------------------------------------------------------------- the layout
def test_the_layout_is_the_mip_layout_in_blocks():
    for W, H in bb.SIZES + ((32768, 1), (1, 32768), (130, 67)):
        for levels in (0, 1, 2):
            if levels > len(lightmap_mip_layout(W, H)):
                continue
            mips, blocks = lightmap_mip_layout(W, H, levels), lightmap_bc6h_layout(W, H, levels)
            assert len(mips) == len(blocks)
            off = 0
            for l, ((w, h, _), (bw, bh, o)) in enumerate(zip(mips, blocks)):
                assert (bw, bh) == (-(-w // 4), -(-h // 4)) and o == (off if l else 0)
                off += bw * bh if l else 0
    for bad in (lambda: lightmap_bc6h_layout(0, 4), lambda: lightmap_bc6h_layout(4, 32769), lambda: lightmap_bc6h_layout(4, 4, 4)):
        with pytest.raises(ValueError):
            bad()
    assert (abi.MI_BC6H_BLOCK_BYTES, abi.MI_BC6H_BLOCK_DIM, abi.MI_BC6H_MODE, abi.MI_BC6H_MAX_ROUNDS) == (16, 4, 3, 4)


def test_the_cpp_plan_is_the_layout(tmp_path):
    so = tmp_path / "bc6h_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-shared",
                    os.path.join(CSRC, "render_plan.cpp"), os.path.join(CSRC, "scene_compile.cpp"),
                    os.path.join(ROOT, "tests", "cpp", "bc6h_plan_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.bc6h_plan_query.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    for W, H in bb.SIZES + ((32768, 32768), (130, 67)):
        for levels in (0, 1, 3):
            out, total = (C.c_uint64 * 48)(), C.c_uint64()
            n = lib.bc6h_plan_query(W, H, levels, out, C.byref(total))
            if levels > len(lightmap_mip_layout(W, H)):
                assert n == -1
                continue
            want = lightmap_bc6h_layout(W, H, levels)
            assert n == len(want) and [tuple(out[3 * l:3 * l + 3]) for l in range(n)] == want
            assert total.value == sum(bw * bh for bw, bh, _ in want[1:])


# ---------------------------------------------------------------- the validator and the lookups
def test_check_refuses_what_the_c_side_refuses():
    W, H = 5, 3
    mips, valids, _ = mb.reference(W, H, 3, "random70")
    chain = lightmap_bc6h_chain(mips, valids)
    uv = lb.points(W, H)[0][:7]
    blocks, checked = check_lightmap_bc6h(chain, W, H, uv, 1.5)
    assert len(blocks) == len(chain) == len(checked[0]) and checked[3].shape == (7,)
    blocks, checked = check_lightmap_bc6h(chain[0], W, H, uv, None, None, abi.MI_LS_NEAREST)
    assert len(blocks) == 1 and checked[3] == abi.MI_LS_NEAREST
    refusals = [
        lambda: check_lightmap_bc6h(chain, W, H, uv),                                             # lod None reads level 0 alone
        lambda: check_lightmap_bc6h(chain[:1], W, H, uv, None, [None, None]),
        lambda: check_lightmap_bc6h(chain, W, H, uv, 0.0, None, abi.MI_LS_NEAREST),                # everything the f32 calls refuse
        lambda: check_lightmap_bc6h(chain + [chain[-1]], W, H, uv, 0.0),
        lambda: check_lightmap_bc6h([chain[0], chain[2], chain[1]], W + 4, H, uv, 0.0),
        lambda: check_lightmap_bc6h(chain[0], W, H, uv, None, None, 2),
        lambda: check_lightmap_bc6h(chain[0], W, H, uv[:, :1]),
        lambda: check_lightmap_bc6h(chain[0], W, H, uv, None, np.ones((H, W + 1))),
        lambda: check_lightmap_bc6h(chain[0], W, H, uv, np.zeros(6)),
        lambda: check_lightmap_bc6h([], W, H, uv),
        lambda: check_lightmap_bc6h(chain[0], 9, H, uv),                                          # the wrong number of blocks
        lambda: check_lightmap_bc6h(chain[0].astype(np.uint16), W, H, uv),
        lambda: lightmap_bc6h_encode(mips[0], None, 5),
        lambda: lightmap_bc6h_encode(mips[0], None, -1),
        lambda: lightmap_bc6h_encode(mips[0][..., :2]),
        lambda: lightmap_bc6h_encode(mips[0], np.ones((H, W + 1))),
        lambda: lightmap_bc6h_chain(mips, valids[:1]),
    ]
    for k, bad in enumerate(refusals):
        with pytest.raises(ValueError):
            bad()
            pytest.fail(f"refusal {k} passed")


@pytest.mark.parametrize("W,H", bb.LOOKUP_SIZES)
def test_a_bc6h_lookup_is_the_f32_lookup_of_the_decoded_chain(W, H):
    for name in bb.LOOKUP_MASKS:
        blocks, valids, levels = bb.chain(W, H, name)
        uv, lod = mb.lod_points(W, H)
        got, want = lightmap_sample_bc6h(blocks, W, H, uv, lod, valids), lightmap_sample_lod(levels, uv, lod, valids)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), name
        pts = lb.points(W, H)[0]
        v0 = None if valids is None else valids[0]
        for flags in (0, abi.MI_LS_NEAREST):
            got, want = lightmap_sample_bc6h(blocks[:1], W, H, pts, None, None if valids is None else valids[:1], flags), lightmap_sample(levels[0], pts, v0, flags)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (name, flags)


# ---------------------------------------------------------------- the C++ mirror, a stand-alone program
@pytest.fixture(scope="module")
def cpp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("bc6h") / "bc6h_lightmap_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "bc6h_lightmap_check.cpp"), "-o", str(exe), "-lz"], check=True)
    return str(exe)


def test_the_cpp_mirror_has_the_helpers_bytes(cpp, tmp_path):
    src, mask, dst = tmp_path / "in.bin", tmp_path / "valid.bin", tmp_path / "out.bin"
    for name, img, valid in bb.encode_batteries():
        H, W = img.shape[:2]
        np.ascontiguousarray(img).tofile(src)
        if valid is not None:
            np.ascontiguousarray(valid).tofile(mask)
        for rounds in bb.ROUNDS:
            r = subprocess.run([cpp, "encode", str(W), str(H), str(rounds), str(src), "-" if valid is None else str(mask), str(dst)], capture_output=True, text=True)
            assert r.returncode == 0, r.stderr
            assert np.array_equal(np.fromfile(dst, np.uint8), bb.reference(name, rounds).reshape(-1)), (name, rounds)
    for name, blocks, W, H in bb.decode_batteries():
        np.ascontiguousarray(blocks).tofile(src)
        r = subprocess.run([cpp, "decode", str(W), str(H), str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert np.array_equal(bits(np.fromfile(dst, f32)), bits(bb.decoded_reference(name).reshape(-1))), name
    for W, H in bb.SIZES:
        r = subprocess.run([cpp, "layout", str(W), str(H), "0"], capture_output=True, text=True)
        assert [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()] == lightmap_bc6h_layout(W, H)
    np.zeros(48, f32).tofile(src)
    for args in (("encode", "4", "4", "5", str(src), "-", str(dst)), ("encode", "5", "4", "2", str(src), "-", str(dst)),
                 ("encode", "0", "4", "2", str(src), "-", str(dst)), ("decode", "8", "8", str(src), str(dst)), ("layout", "4", "4", "9")):
        r = subprocess.run([cpp, *args], capture_output=True, text=True)
        assert r.returncode == 1 and "mi_rt" in r.stderr, args


# ---------------------------------------------------------------- mutants
def test_the_mutant_machinery_changes_nothing():
    same = ("better = cerr < err",) * 2
    copy = bb.mutant(lightmap_bc6h_encode, bb.ENCODE_BLOCKS, *same)
    assert copy is not lightmap_bc6h_encode and bb.encode_differs(copy) == []


@pytest.mark.parametrize("name", sorted(bb.ENCODE_MUTANTS))
def test_batteries_notice_encoder_mutants(name):
    found = bb.encode_differs(bb.mutant(lightmap_bc6h_encode, bb.ENCODE_BLOCKS, *bb.ENCODE_MUTANTS[name]))
    assert found, name


def test_the_equivalent_mutant_is_equivalent():
    """floor for ceil in the start's domain map changes no field, for any h: bc6h_batteries.EQUIVALENT_MUTANTS says why"""
    h = np.arange(0, 0x7C00, dtype=np.int64)
    assert np.array_equal(tracing._bc6h_quant((64 * h + 30) // 31), tracing._bc6h_quant((64 * h) // 31))
    for name, (old, new) in bb.EQUIVALENT_MUTANTS.items():
        assert bb.encode_differs(bb.mutant(lightmap_bc6h_encode, bb.ENCODE_BLOCKS, old, new)) == [], name
