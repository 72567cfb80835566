"""Lightmap mips on the host: the layout (lightmap_mip_layout against render_plan.cpp mip_plan, asked through tests/cpp/mip_plan_shim.cpp),
the numpy definitions lightmap_mips, lightmap_sample_lod and lightmap_sh_sample_lod (tracing.py) against what they must agree with, and
the batteries of tests/mips_batteries.py shown to notice one-token mutants of the definitions (so that a kernel which implemented a mutant
could not equal the helper on all of them).  No GPU.

Bounds.  Pyramid: level l is held to the float64 mean over the valid level-0 texels of its footprint within
5 l 2^-24 x (mean of |t| over them): per level the product c t, three sums and the quotient are five roundings of terms whose absolute
values average to that mean, and the roundings of the levels below pass through with weights that sum to one.
Trilinear lookup, plain form: 1 - f on both axes and between the levels (3), w_x w_y and w_level (..) (2) and w t (1) are 6 roundings
per term, up to 7 further adds of acc: 13 on the numerator; the weights' 5 and 7 adds of sw on the denominator: 12; one division:
|helper - f64| <= 27 * 2^-24 * max|t| (gamma_26, first order, rounded up).  out_weight: |sw - 1| <= 12 * 2^-24 where every tap is valid.
SH form: the 56 roundings lightmap_sh_sample's bound leaves to the evaluation of one tap and the 26 above stay below 96 roundings of terms
that sum to sum_taps w sum_k |B_k r_k| / sw, per channel (B_k: mips_batteries.f64_lookup_lod).

One mutant of the issue's list is EQUIVALENT and is shown to be: dropping `min(.., max(L - 2, 0))` changes l_a only where lam is L - 1
exactly, from (l_a, f) = (L - 2, 1) to (L - 1, 0); level a then has weight 0 in the first form and level b in the second, so both read
the same single level L - 1 with level weight 1 and the same four taps in the same order: no input can tell them apart.
test_the_last_level_rule_is_a_choice_of_form asserts that equality instead of a difference."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cs397raytracingsp22_amd as pkg
from cs397raytracingsp22_amd import (abi, check_lightmap_lod, check_lightmap_mips, lightmap_mip_layout, lightmap_mips, lightmap_sample,
                                     lightmap_sample_lod, lightmap_sh_sample, lightmap_sh_sample_lod)

import finish_batteries as fb
import lookup_batteries as lb
import mips_batteries as mb
from mips_batteries import CHANNELS, FORMS, LOD_MASKS, LOD_SIZES, MASKS, SIZES, bits, f32

EPS = 2.0 ** -24
CSRC = os.path.join(fb.ROOT, "cs397raytracingsp22_amd", "csrc")


# ---------------------------------------------------------------- the layout, and the C++ plan
class MipPlanQuery(C.Structure):           # tests/cpp/mip_plan_shim.cpp
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("levels", C.c_uint32), ("per_launch", C.c_uint32),
                ("n_levels", C.c_uint32), ("full_chain", C.c_uint32), ("texels", C.c_uint64),
                ("level_size", C.c_uint32 * 32), ("level_offset", C.c_uint64 * 16), ("launches", C.c_uint32 * 32)]


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    so = tmp_path_factory.mktemp("mp") / "mip_plan_shim.so"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-fPIC", "-shared",
                    os.path.join(CSRC, "render_plan.cpp"), os.path.join(CSRC, "scene_compile.cpp"),
                    os.path.join(fb.ROOT, "tests", "cpp", "mip_plan_shim.cpp"), "-o", str(so)], check=True)
    lib = C.CDLL(str(so))
    lib.mip_plan_query.argtypes = [C.POINTER(MipPlanQuery)]
    lib.mip_plan_query.restype = C.c_int

    def plan(W, H, levels=0, per_launch=5):
        """([(W_l, H_l, offset_l)], texels of levels 1 .., [(level read, levels written)]) or None: refused"""
        q = MipPlanQuery(width=W, height=H, levels=levels, per_launch=per_launch)
        n = lib.mip_plan_query(C.byref(q))
        if n < 0:
            return None
        assert q.full_chain == len(lightmap_mip_layout(W, H))
        layout = [(q.level_size[2 * l], q.level_size[2 * l + 1], q.level_offset[l]) for l in range(q.n_levels)]
        return layout, q.texels, [(q.launches[2 * i], q.launches[2 * i + 1]) for i in range(n)]
    return plan


def test_the_layout_is_iterated_ceil_halving():
    for W, H in SIZES + ((32768, 1), (1, 32768), (32768, 32768), (32767, 5)):
        layout = lightmap_mip_layout(W, H)
        w, h, off = W, H, 0
        for l, (wl, hl, ol) in enumerate(layout):
            assert (wl, hl) == (w, h) and ol == (off if l else 0), (W, H, l)
            off += wl * hl if l else 0
            w, h = (w + 1) // 2, (h + 1) // 2
        assert layout[-1][:2] == (1, 1) and (len(layout) == 1 or layout[-2][:2] != (1, 1))          # the full chain ends at 1 x 1, once
        assert len(layout) == 1 + int(np.ceil(np.log2(max(W, H))))
        for levels in range(1, len(layout) + 1):
            assert lightmap_mip_layout(W, H, levels) == layout[:levels]
        assert lightmap_mip_layout(W, H, 0) == layout
    assert len(lightmap_mip_layout(32768, 32768)) == 16 and len(lightmap_mip_layout(130, 67)) == 9
    for bad in ((0, 1, 0), (1, 0, 0), (32769, 1, 0), (1, 32769, 0), (4, 4, 4), (1, 1, 2), (130, 67, 10), (8, 8, -1)):
        with pytest.raises(ValueError):
            lightmap_mip_layout(*bad)


def test_the_cpp_plan_agrees_and_writes_every_level_once(plan):
    for W, H in SIZES + ((32768, 1), (32768, 32768)):
        layout = lightmap_mip_layout(W, H)
        for levels in (0, 1, len(layout), max(len(layout) - 1, 1)):
            want = lightmap_mip_layout(W, H, levels)
            for per_launch in (5, 1, 2, 0, 9):
                got, texels, launches = plan(W, H, levels, per_launch)
                assert got == want and texels == sum(w * h for w, h, _ in want[1:]), (W, H, levels)
                cap = min(max(per_launch, 1), 5)
                written, src = [], 0
                for read, count in launches:
                    assert read == src and 1 <= count <= cap, (W, H, levels, per_launch)      # a launch reads the last level the one before wrote
                    written += list(range(read + 1, read + 1 + count))
                    src = read + count
                assert written == list(range(1, len(want))), (W, H, levels, per_launch)
                assert len(launches) == -(-(len(want) - 1) // cap)
        assert plan(W, H, len(layout) + 1) is None                                                # above the full chain
    assert [c for _, c in plan(130, 67)[2]] == [5, 3] and plan(1, 1)[2] == [] and len(plan(32768, 32768)[2]) == 3
    for bad in ((0, 4), (4, 0), (32769, 4), (4, 32769)):
        assert plan(*bad) is None


# ---------------------------------------------------------------- the check functions
def test_check_refuses_what_the_c_side_refuses():
    img = np.zeros((5, 3, 3), f32)
    out = check_lightmap_mips(img)
    assert out[0].shape == (5, 3, 3) and out[1] is None and len(out[2]) == 4
    assert check_lightmap_mips(np.zeros((5, 3, 9, 3)), np.ones((5, 3)), 2)[0].shape == (5, 3, 27)
    for args in ((np.zeros((5, 3)),), (np.zeros((5, 3, 4)),), (np.zeros((0, 3, 3)),), (np.zeros((1, 32769, 3)),), (img, np.ones((3, 5))),
                 (img, None, 5), (img, None, -1)):
        with pytest.raises(ValueError):
            check_lightmap_mips(*args)
        with pytest.raises(ValueError):
            lightmap_mips(*args)
    chain, valids, _ = lightmap_mips(img, np.ones((5, 3)))
    uv = np.zeros((7, 2), f32)
    got = check_lightmap_lod(chain, uv, 0.5, valids)
    assert len(got[0]) == 4 and got[3].shape == (7,) and got[5] == (7,)
    assert check_lightmap_lod(chain[:1], uv, np.zeros(7))[1] == [None]
    assert check_lightmap_lod(chain, uv, 0.0, [None] + valids[1:])[1][0] is None
    bad = [
        (chain, uv, 0.0, None, abi.MI_LS_NEAREST), (chain, uv, 0.0, None, 2), (chain, uv, 0.0, None, 0x80000000),
        ([], uv, 0.0), (img, uv, 0.0), (chain + [chain[-1]], uv, 0.0), ([chain[0], chain[2]], uv, 0.0), ([np.zeros((5, 3, 4), f32)], uv, 0.0),
        (chain, np.zeros((7, 3)), 0.0), (chain, uv, np.zeros(6)), (chain, uv, np.zeros((7, 1))),
        (chain, uv, 0.0, valids[:2]), (chain, uv, 0.0, [valids[0], valids[1], None, None]), (chain, uv, 0.0, [valids[1]] + valids[1:]),
        (chain, uv, 0.0, None, 0, np.zeros((6, 3))),
    ]
    for args in bad:
        with pytest.raises(ValueError):
            check_lightmap_lod(*args)
        if len(args) < 6:
            with pytest.raises(ValueError):
                lightmap_sample_lod(*args)
    with pytest.raises(ValueError):
        lightmap_sh_sample_lod(chain, uv, np.zeros((7, 3)), 0.0)                  # three channels are no SH records
    with pytest.raises(ValueError):
        lightmap_sh_sample_lod(chain, uv, None, 0.0)


# ---------------------------------------------------------------- the pyramid
@pytest.mark.parametrize("W,H", SIZES)
def test_coverage_is_the_valid_fraction_of_the_footprint(W, H):
    for name in MASKS:
        valid = mb.mask(W, H, name)
        ok = np.ones((H, W), bool) if valid is None else valid != 0
        mips, valids, covs = mb.reference(W, H, 3, name)
        assert len(mips) == len(lightmap_mip_layout(W, H)) and mips[0] is not None
        for l, (wl, hl, _) in enumerate(lightmap_mip_layout(W, H)):
            count = mb.footprint_sums(ok.astype(np.float64), l)
            assert covs[l].shape == (hl, wl) == valids[l].shape and mips[l].shape == (hl, wl, 3)
            assert np.array_equal(covs[l].astype(np.float64), count / 4.0 ** l), (W, H, name, l)        # exact: l <= 8 here
            assert np.array_equal(valids[l] != 0, count > 0)
        assert np.array_equal(bits(covs[-1]), bits(mb.reference(W, H, 27, name)[2][-1]))                # the channel count changes no coverage


@pytest.mark.parametrize("W,H", SIZES)
def test_every_level_is_the_mean_over_the_valid_footprint(W, H):
    worst = 0.0
    for C_ in CHANNELS:
        for name in MASKS:
            img, valid = mb.masked(W, H, C_, name)
            mips = mb.reference(W, H, C_, name)[0]
            for l in range(1, len(mips)):
                want, count, mean_abs = mb.f64_mips(img, valid, l)
                got = mips[l].astype(np.float64)
                live = count > 0
                assert np.isfinite(got).all()                                                          # the gutters' poison reaches nothing
                assert np.array_equal(bits(mips[l][~live]), np.zeros(((~live).sum(), C_), np.uint32))    # nothing valid below: +0
                err, room = np.abs(got - want)[live], (5 * l * EPS * mean_abs)[live]
                assert (err <= room).all(), (W, H, C_, name, l, float((err / np.maximum(room, 1e-300)).max()))
                if (room > 0).any():
                    worst = max(worst, float((err[room > 0] / (EPS * mean_abs[live][room > 0])).max()))
    print(f"{W} x {H}: the worst error is {worst:.2f} x 2^-24 x the mean of |t|")


def test_sub_chains_are_prefixes_of_the_full_chain():
    for W, H in ((33, 45), (130, 67)):
        img, valid = mb.masked(W, H, 3, "random70")
        full = mb.reference(W, H, 3, "random70")
        for levels in (1, 2, 6, 7):
            assert mb.same_chain(lightmap_mips(img, valid, levels), tuple(part[:levels] for part in full))


def test_a_constant_image_comes_back_constant():
    c = np.array([0.3, -1.7, 1234.5], f32)
    mips, _, _ = lightmap_mips(np.broadcast_to(c, (64, 64, 3)))
    for level in mips:                                               # all valid, a power of two: every sum and quotient is exact
        assert np.array_equal(bits(level), bits(np.broadcast_to(c, level.shape)))
    for W, H in SIZES:
        for name in MASKS:
            mips, valids, _ = lightmap_mips(np.broadcast_to(c, (H, W, 3)), mb.mask(W, H, name))
            for l in range(1, len(mips)):
                live = valids[l] != 0
                assert (np.abs(mips[l][live].astype(np.float64) - c) <= 5 * l * EPS * np.abs(c)).all(), (W, H, name, l)
                assert not mips[l][~live].any()


def test_poison_behind_the_mask_changes_no_bit():
    for W, H in SIZES:
        for C_ in CHANNELS:
            img, valid = mb.masked(W, H, C_, "charts")
            assert (valid == 0).sum() == 0 or np.isnan(img[valid == 0]).any()
            clean = np.where((valid != 0)[..., None], img, f32(0.0))
            got, want = lightmap_mips(clean, valid), mb.reference(W, H, C_, "charts")
            assert mb.same_chain([part[1:] for part in got], [part[1:] for part in want])              # (level 0 is the image itself)


def test_a_valid_nan_reaches_exactly_its_ancestors():
    for W, H in ((33, 45), (130, 67), (3, 5)):
        img, valid = mb.masked(W, H, 3, "random70")
        y, x = np.argwhere(valid != 0)[len(np.argwhere(valid != 0)) // 2]
        spoiled = img.copy()
        spoiled[y, x, 1] = f32(np.nan)
        got, want = lightmap_mips(spoiled, valid), mb.reference(W, H, 3, "random70")
        assert mb.same_chain(got[1:], want[1:])                                        # masks and coverage do not look at the values
        for l in range(1, len(want[0])):
            hit = np.zeros(want[0][l].shape, bool)
            hit[y >> l, x >> l, 1] = True
            assert np.array_equal(np.isnan(got[0][l]), hit), (W, H, l)
            assert np.array_equal(bits(got[0][l][~hit]), bits(want[0][l][~hit]))


# ---------------------------------------------------------------- the trilinear lookup: the identities
def _lookup(form, chain, uv, lod, valids, nrm):
    return lightmap_sh_sample_lod(chain, uv, nrm, lod, valids) if form == "sh" else lightmap_sample_lod(chain, uv, lod, valids)


def _level_lookup(form, img, uv, valid, nrm):
    return lightmap_sh_sample(img, uv, nrm, valid) if form == "sh" else lightmap_sample(img, uv, valid)


@pytest.mark.parametrize("W,H", LOD_SIZES)
def test_level_zero_is_the_bilinear_lookup(W, H):
    """With one level, lod <= 0 or a NaN lod the result is lightmap_sample / lightmap_sh_sample of level 0, bit for bit, at any size"""
    for form in FORMS:
        for name in LOD_MASKS:
            chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, name)
            out, sw = mb.lod_reference(W, H, form, name)
            want = _level_lookup(form, chain[0], uv, None if valids is None else valids[0], nrm)
            low = ~(lod > 0)                                                              # lod <= 0 and NaN
            assert low.sum() >= len(lod) // 4
            assert np.array_equal(bits(out[low]), bits(want[0][low])) and np.array_equal(bits(sw[low]), bits(want[1][low])), (form, name)
            one = _lookup(form, chain[:1], uv, lod, None if valids is None else valids[:1], nrm)
            assert np.array_equal(bits(one[0]), bits(want[0])) and np.array_equal(bits(one[1]), bits(want[1])), (form, name)


def test_an_integer_lod_is_the_bilinear_lookup_of_that_level():
    """At an integer lod = l on a size divisible by 2^l the result is lightmap_sample of level l with that level's mask, bit for bit"""
    for W, H, top in ((64, 64, 6), (96, 32, 5)):
        uv = lb.points(W, H)[0][::3]
        nrm = lb.normals(len(uv))
        for form in FORMS:
            for name in LOD_MASKS:
                img = mb.image(W, H, 3 if form == 3 else 27)
                chain, valids, _ = lightmap_mips(img, mb.mask(W, H, name))
                for l in range(top + 1):
                    got = _lookup(form, chain, uv, f32(l), valids, nrm)
                    want = _level_lookup(form, chain[l], uv, valids[l], nrm)
                    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), (W, H, form, name, l)


# ---------------------------------------------------------------- the trilinear lookup: the float64 restatement
def assert_within(got, want, scale, factor, clean, what):
    """|got - want| <= factor 2^-24 scale wherever want is finite, the same non-finite places, on the `clean` points"""
    got, want = got[clean].astype(np.float64), want[clean]
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), what
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    room = np.where(fin, factor * EPS * np.broadcast_to(scale[clean], err.shape), 0.0)
    assert (err <= room).all(), (what, float((err[fin] / np.maximum(room[fin], 1e-300)).max()))


@pytest.mark.parametrize("W,H", LOD_SIZES)
def test_the_helpers_against_the_f64_restatement(W, H):
    for form in FORMS:
        for name in LOD_MASKS:
            chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, form, name)
            want, wsw, scale = mb.f64_lookup_lod(chain, valids, uv, lod, nrm)
            out, sw = mb.lod_reference(W, H, form, name)
            clean = lb.clean_normals(len(uv)) if form == "sh" else np.ones(len(uv), bool)
            assert_within(out, want, scale, 96 if form == "sh" else 27, clean, (W, H, form, name))
            assert (np.abs(sw - wsw)[clean] <= 12 * EPS).all()
            assert np.isfinite(out[clean]).all()                                       # the gutters' poison reaches nothing
            if name == "null":                                                          # every tap valid: the weight is 1 within rounding
                assert (np.abs(sw[clean].astype(np.float64) - 1.0) <= 12 * EPS).all()
            fractional = (lod > 0) & (lod < len(chain) - 1) & (lod != np.floor(lod))
            assert fractional.any() == (len(chain) > 1)


def test_shapes_pass_through():
    W, H = 33, 45
    chain, valids, uv, lod, nrm = mb.lod_inputs(W, H, "sh", "random70")
    E, sw = mb.lod_reference(W, H, "sh", "random70")
    for n in lb.COUNTS:
        e, s = lightmap_sh_sample_lod(chain, uv[:n], nrm[:n], lod[:n], valids)
        assert e.shape == (n, 3) and np.array_equal(bits(e), bits(E[:n])) and np.array_equal(bits(s), bits(sw[:n]))
    e, s = lightmap_sh_sample_lod([a.reshape(a.shape[:2] + (9, 3)) for a in chain], uv[:12].reshape(3, 4, 2), nrm[:12].reshape(3, 4, 3),
                                  lod[:12].reshape(3, 4), valids)
    assert e.shape == (3, 4, 3) and s.shape == (3, 4) and np.array_equal(bits(e).reshape(12, 3), bits(E[:12]))
    o, s = lightmap_sample_lod(chain, uv[:12].reshape(2, 6, 2), 1.5, valids)                  # a scalar lod serves every point
    assert o.shape == (2, 6, 27) and np.array_equal(bits(o).reshape(12, 27), bits(lightmap_sample_lod(chain, uv[:12], np.full(12, 1.5), valids)[0]))
    assert lightmap_sample_lod(chain, uv[:0], lod[:0])[0].shape == (0, 27)


# ---------------------------------------------------------------- mutants
def test_the_mutant_machinery_changes_nothing():
    same = ("for dy, dx in _LMM_CHILDREN:",) * 2
    copy = mb.mutant(lightmap_mips, mb.MIPS_BLOCKS, *same)
    assert copy is not lightmap_mips and not mb.mips_differs(copy, SIZES[:5])
    same = ("(f32(1.0) - fl, fl)",) * 2
    assert not mb.lod_differs(mb.mutant(lightmap_sample_lod, mb.LOD_BLOCKS, *same), 27, LOD_SIZES[:4])
    assert not mb.lod_differs(mb.mutant(lightmap_sh_sample_lod, mb.LOD_BLOCKS, *same), "sh", LOD_SIZES[:4])


@pytest.mark.parametrize("name", sorted(mb.MIPS_MUTANTS))
def test_batteries_notice_pyramid_mutants(name):
    assert mb.mips_differs(mb.mutant(lightmap_mips, mb.MIPS_BLOCKS, *mb.MIPS_MUTANTS[name]))


@pytest.mark.parametrize("name", sorted(mb.LOD_MUTANTS))
def test_batteries_notice_lookup_mutants(name):
    assert mb.lod_differs(mb.mutant(lightmap_sample_lod, mb.LOD_BLOCKS, *mb.LOD_MUTANTS[name]), 3)
    assert mb.lod_differs(mb.mutant(lightmap_sh_sample_lod, mb.LOD_BLOCKS, *mb.LOD_MUTANTS[name]), "sh")


def test_the_last_level_rule_is_a_choice_of_form():
    """Without min(.., max(L - 2, 0)) the one place that changes, lam == L - 1, reads the same level with the same weights: an equivalent
    mutant (module docstring).  The batteries do reach that place."""
    for W, H in LOD_SIZES:
        lod = mb.lod_points(W, H)[1]
        assert (np.fmin(np.fmax(lod, f32(0)), f32(mb.full_chain(W, H) - 1)) == f32(mb.full_chain(W, H) - 1)).any()
    assert not mb.lod_differs(mb.mutant(lightmap_sample_lod, mb.LOD_BLOCKS, *mb.LAST_LEVEL), 27)
    assert not mb.lod_differs(mb.mutant(lightmap_sh_sample_lod, mb.LOD_BLOCKS, *mb.LAST_LEVEL), "sh")


# ---------------------------------------------------------------- the mirrors
def test_the_prototypes_and_the_names_are_declared():
    lib = abi.load()
    for name, argc in (("mi_lightmap_mips", 10), ("mi_lightmap_mips_device", 11), ("mi_lightmap_sample_lod", 15),
                       ("mi_lightmap_sample_lod_device", 16), ("mi_lightmap_sh_sample_lod", 15), ("mi_lightmap_sh_sample_lod_device", 16)):
        assert name in abi.EXPORTS and len(getattr(lib, name).argtypes) == argc, name
        assert getattr(lib, name).restype is C.c_int
    for name in ("lightmap_mip_layout", "lightmap_mips", "lightmap_sample_lod", "lightmap_sh_sample_lod", "check_lightmap_mips",
                 "check_lightmap_lod"):
        assert name in pkg.__all__ and callable(getattr(pkg, name)), name
    for name in ("lightmap_mips", "lightmap_mips_device", "lightmap_sample_lod", "lightmap_sample_lod_device", "lightmap_sh_sample_lod",
                 "lightmap_sh_sample_lod_device"):
        assert callable(getattr(pkg.Context, name)), name
    hdr = open(fb.ROOT + "/include/mi_rt.h").read()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)
    hpp = open(fb.ROOT + "/cs397raytracingsp22_amd/host/tracing.hpp").read()
    rs = open(fb.ROOT + "/rust/src/util/tracing_flatten.rs").read()
    for name in ("lightmap_mips", "sample_lightmap_lod", "sample_lightmap_sh_lod", "lightmap_mip_layout"):
        assert re.search(r"static std::vector<\w+> " + name + r"\(", hpp), name
        assert re.search(r"pub fn " + name + r"\(", rs), name
    for name in ("mi_lightmap_mips", "mi_lightmap_sample_lod", "mi_lightmap_sh_sample_lod"):
        assert name + "(" in hpp and "mi_rt::" + name + "(" in rs, name
