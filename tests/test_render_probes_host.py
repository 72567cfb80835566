"""Light probes (mi_render_probes / mi_render_probes_device): what can be checked without a GPU — the numpy SH helpers against an exact
f64 quadrature of the sphere, probe_grid, the Python input checking, and the two prototypes in the header, the ctypes mirror, the C++
mirror and the Rust text with identical parameter lists.

The quadrature: Gauss-Legendre in t = cos(theta) about the +y axis times a uniform grid in the azimuth, weights summing to 4 pi.  With 16
nodes and 32 azimuths it integrates every product of two basis functions (polynomials of degree <= 4 in x, y, z) exactly; the clamped
cosine about +y is a polynomial in t on t >= 0, so the same rule over [0, 1] integrates its products with the basis exactly too."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from test_render_points_host import HEAD, STATS, U32, VP, _c_types, _header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_render_probes", "mi_render_probes_device"]
TABLE = [("const float*", "*const f32", "c_void_p"), U32]
F32P = ("float*", "*mut f32", "c_void_p")
PARAMS = {
    "mi_render_probes": HEAD + TABLE + [F32P, F32P, ("uint8_t*", "*mut u8", "c_void_p"), ("uint32_t*", "*mut u32", "c_void_p"), STATS],
    "mi_render_probes_device": HEAD + TABLE + [U32, U32, VP, VP, VP, VP, VP, STATS],
}


# ---------------------------------------------------------------- the SH helpers
def sphere_rule(t_lo=-1.0, t_hi=1.0, n_t=16, n_phi=32):
    """(directions [n, 3], weights [n]) integrating over the part of the sphere with t_lo <= y <= t_hi"""
    t, wt = np.polynomial.legendre.leggauss(n_t)
    t = 0.5 * (t_hi - t_lo) * t + 0.5 * (t_hi + t_lo)
    wt = 0.5 * (t_hi - t_lo) * wt
    phi = (np.arange(n_phi) + 0.5) * (2.0 * np.pi / n_phi)
    s = np.sqrt(1.0 - t * t)
    d = np.stack([np.outer(s, np.cos(phi)), np.outer(t, np.ones(n_phi)), np.outer(s, np.sin(phi))], axis=-1).reshape(-1, 3)
    w = np.outer(wt, np.full(n_phi, 2.0 * np.pi / n_phi)).reshape(-1)
    return d, w


def test_sh9_basis_is_orthonormal():
    from cs397raytracingsp22_amd import sh9_basis
    d, w = sphere_rule()
    assert abs(w.sum() - 4.0 * np.pi) <= 1e-12
    Y = sh9_basis(d)
    assert Y.shape == (len(d), 9) and Y.dtype == np.float64
    gram = (Y * w[:, None]).T @ Y
    err = float(np.abs(gram - np.eye(9)).max())
    print(f"sh9_basis: max |<Y_i, Y_j> - delta_ij| = {err:.2e}")
    assert err <= 1e-10
    # the stated order and constants, at directions that tell the nine apart; any length of the argument (it is normalised)
    for v, k, val in (((0, 2, 0), 1, 0.4886025119029199), ((0, 0, 3), 2, 0.4886025119029199), ((0.5, 0, 0), 3, 0.4886025119029199),
                      ((0, 0, 1), 6, 2 * 0.31539156525252005), ((1, 0, 0), 6, -0.31539156525252005), ((1, 0, 0), 8, 0.5462742152960396),
                      ((0, 1, 0), 8, -0.5462742152960396), ((1, 1, 0), 4, 0.5 * 1.0925484305920792), ((0, 1, 1), 5, 0.5 * 1.0925484305920792),
                      ((1, 0, 1), 7, 0.5 * 1.0925484305920792), ((0.3, -0.2, 0.9), 0, 0.28209479177387814)):
        assert abs(sh9_basis(np.float64(v))[k] - val) <= 1e-12, (v, k)
    assert sh9_basis(np.zeros((4, 5, 3)) + (0, 0, 1)).shape == (4, 5, 9)


def test_sh9_irradiance_of_constant_radiance_is_pi_L():
    from cs397raytracingsp22_amd import sh9_basis, sh9_irradiance
    d, w = sphere_rule()
    L = np.float64([1.0, 2.0, 0.25])
    sh = ((sh9_basis(d) * w[:, None]).sum(axis=0))[:, None] * L                     # c_k = integral of L Y_k: only c_0 survives
    assert np.abs(sh[1:]).max() <= 1e-12 and np.allclose(sh[0], np.sqrt(4.0 * np.pi) * L, rtol=0, atol=1e-12)
    for n in ((0, 1, 0), (0, -1, 0), (1, 0, 0), (0.3, -0.5, 0.8), (-2, 1, 7)):
        assert np.abs(sh9_irradiance(sh, n) - np.pi * L).max() <= 1e-12, n
    # one normal per probe broadcasts
    many = sh9_irradiance(np.broadcast_to(sh, (6, 9, 3)), np.random.default_rng(1).normal(size=(6, 3)))
    assert many.shape == (6, 3) and np.abs(many - np.pi * L).max() <= 1e-12


def test_sh9_irradiance_of_a_clamped_cosine_lobe():
    """L(w) = max(0, w.y).  Its order-2 expansion is 1/4 + 1/2 cos + 5/16 (3 cos^2 - 1)/2 in the angle to +y (Ramamoorthi & Hanrahan's
    A_l / pi), and convolving once more with the cosine gives E(+-y) = pi/4 +- pi/3 + 5 pi/64 (the exact values are 2 pi/3 and 0)."""
    from cs397raytracingsp22_amd import sh9_basis, sh9_irradiance
    d, w = sphere_rule(0.0, 1.0)
    sh = (sh9_basis(d) * (w * d[:, 1])[:, None]).sum(axis=0)[:, None]              # one channel
    assert abs(sh[0, 0] - 0.28209479177387814 * np.pi) <= 1e-12 and abs(sh[1, 0] - 0.4886025119029199 * 2.0 * np.pi / 3.0) <= 1e-12
    up, down = sh9_irradiance(sh, (0, 1, 0))[0], sh9_irradiance(sh, (0, -1, 0))[0]
    print(f"clamped cosine: E(+y) = {up:.12f}, E(-y) = {down:.12f}")
    assert abs(up - (np.pi / 4 + np.pi / 3 + 5 * np.pi / 64)) <= 1e-12
    assert abs(down - (np.pi / 4 - np.pi / 3 + 5 * np.pi / 64)) <= 1e-12
    assert abs(up - 2 * np.pi / 3) < 0.02 and abs(down) < 0.02                     # and that approximation is a good one


def test_probe_grid_shapes_and_padding():
    from cs397raytracingsp22_amd import probe_grid
    pts, n = probe_grid((-1, 0, 2), (1, 4, 8), (2, 4, 3))                          # default width: the multiple of 32 above sqrt(n)
    assert n == 24 and pts.shape == (1, 32, 3) and pts.dtype == np.float32 and pts.flags["C_CONTIGUOUS"]
    flat = pts.reshape(-1, 3)[:24]
    assert np.array_equal(pts[0, 24:], np.repeat(flat[-1:], 8, axis=0))            # padding repeats the last probe
    assert np.allclose(flat[0], (-0.5, 0.5, 3.0)) and np.allclose(flat[1], (0.5, 0.5, 3.0))          # cell centres, x fastest
    assert np.allclose(flat[2], (-0.5, 1.5, 3.0)) and np.allclose(flat[8], (-0.5, 0.5, 5.0)) and np.allclose(flat[23], (0.5, 3.5, 7.0))
    pts, n = probe_grid((-1, 0, 2), (1, 4, 8), (2, 4, 3), width=7)                 # 24 probes in 4 rows of 7: four padding slots
    assert n == 24 and pts.shape == (4, 7, 3)
    assert np.array_equal(pts.reshape(-1, 3)[:24], flat) and np.array_equal(pts.reshape(-1, 3)[24:], np.repeat(flat[-1:], 4, axis=0))
    assert probe_grid((0, 0, 0), (1, 1, 1), (1, 1, 1), width=1)[0].tolist() == [[[0.5, 0.5, 0.5]]]
    big, n = probe_grid((0, 0, 0), (1, 1, 1), (40, 40, 40))
    assert n == 64000 and big.shape == (250, 256, 3) and np.isfinite(big).all()
    assert probe_grid((0, 0, 0), (1, 1, 1), (64, 4, 4), width=1024)[0].shape == (1, 1024, 3)
    for bad in (dict(counts=(0, 1, 1)), dict(counts=(2, 2, 2), width=0), dict(counts=(2, 2, 2), width=40000)):
        with pytest.raises(ValueError):
            probe_grid((0, 0, 0), (1, 1, 1), **bad)


# ---------------------------------------------------------------- the Python mirror's checks
def _cam(**kw):
    from cs397raytracingsp22_amd import Camera
    base = dict(screen_width=7, screen_height=5, aa_sample_count=4, path_depth=6)
    base.update(kw)
    return Camera(**base)


def _table(s, h=5, w=7, dtype=np.float32):
    return np.zeros((s, h, w, 3) if s else (h, w, 3), dtype)


def test_check_probe_table():
    from cs397raytracingsp22_amd.tracing import ShadingMode, check_probe_table
    cam = _cam()
    for s, rows in ((0, 1), (4, 4), (1, 1)):
        p, r = check_probe_table(cam, _table(s))
        assert r == rows and p.shape == (rows, 5, 7, 3) and p.dtype == np.float32 and p.flags["C_CONTIGUOUS"]
    assert check_probe_table(_cam(aa_sample_count=5), _table(5))[1] == 5           # a non-square aa is fine
    nan = float("nan")
    bad = _table(0)
    bad[1, 1] = (nan, 0.0, float("inf"))                                           # values are not the checker's business
    assert check_probe_table(_cam(eyepoint=(nan, nan, nan)), bad)[1] == 1
    for p in (_table(4, dtype=np.float64), _table(4, h=7, w=5), _table(0, h=5, w=8), _table(2), np.zeros((5, 7), np.float32)):
        with pytest.raises(ValueError):
            check_probe_table(cam, p)
    for kw in (dict(path_samples=2), dict(path_samples=0), dict(shading_mode=ShadingMode.Phong), dict(max_trace_dist=nan), dict(gamma=0.0),
               dict(aa_sample_count=0), dict(screen_width=40000)):
        with pytest.raises(ValueError):
            check_probe_table(_cam(**kw), _table(0))
    with pytest.raises(ValueError, match="points must be float32"):
        check_probe_table(cam, _table(4, dtype=np.float64))
    with pytest.raises(ValueError, match="a probe table holds 1 row or aa_sample_count = 4 rows"):
        check_probe_table(cam, _table(2))


def test_render_probes_refuses_before_any_library_call():
    from cs397raytracingsp22_amd import Context, Scene
    ctx = Context.__new__(Context)                        # no mi_ctx_create: any library call would fail on the missing handle
    with pytest.raises(ValueError):
        Context.render_probes(ctx, _cam(), _table(2))
    with pytest.raises(ValueError):
        Context.render_probes(ctx, _cam(), _table(4, dtype=np.float64))
    with pytest.raises(ValueError):
        Scene(_cam(path_samples=2), []).render_probes(_table(4))


# ---------------------------------------------------------------- the symbols, in the header and the three mirrors
def test_header_declares_both_with_the_stated_parameter_lists(tmp_path):
    hdr = _header()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)           # additive: the version did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        args = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code).group(1)
        assert _c_types(args) == [p[0] for p in PARAMS[name]], name
    src = tmp_path / "pr.c"
    src.write_text('#include "mi_rt.h"\nint main(void) {\n' + "".join(
        f"    int (*f{k})({', '.join(p[0] for p in PARAMS[n])}) = {n};\n" for k, n in enumerate(NAMES)) + "    return f0 == 0 || f1 == 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "pr.o")],
                   check=True)
    doc = " ".join(re.sub(r"\n \*", "\n", hdr[hdr.index("---- light probes"):hdr.index("int  mi_render_probes(")]).split())
    for phrase in ("[rows_per_pixel][H][W][3]", "(seed, W*H + y*W + x, s)", "(seed, y*W + x, s)", "rand_sphere_vec", "materials.rs:158-166",
                   "NOT normalised", "|d| <= 1", "t_min = 0.001", "[H][W][9][3]", "(4 pi / S)", "0.28209479177387814", "0.4886025119029199",
                   "1.0925484305920792", "0.31539156525252005", "0.5462742152960396", "in sample order", "12.566370614359172f",
                   "bit-identical", "No empty-probe marker", "never faults", "that probe only", "dot(d, d) == 0", "unspecified",
                   "[tiles_padded][1024][27]", "sample_begin == 0", "need not be cleared", "written as zeros",
                   "d_compact_sh == NULL is legal", "out_sh is required", "mi_multi_* takes no table"):
        assert phrase in doc, phrase


def test_ctypes_mirror_has_the_same_parameter_lists():
    from cs397raytracingsp22_amd import abi
    lib = abi.load()
    for name in NAMES:
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == len(PARAMS[name]), name
        for k, (t, p) in enumerate(zip(fn.argtypes, PARAMS[name])):
            assert (t is getattr(C, p[2])) if hasattr(C, p[2]) else (t.__name__ == p[2]), (name, k, t, p[2])
    raw = C.CDLL(abi.LIB_PATH)                            # a fresh handle: no prototypes of the mirror involved
    for name in NAMES:
        assert C.cast(getattr(raw, name), C.c_void_p).value


def test_rust_and_cpp_mirrors_have_the_same_parameter_lists(tmp_path):
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        args = re.search(rf"pub\s+fn\s+{name}\s*\(([^)]*)\)\s*->\s*c_int;", block).group(1)
        types = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",")]
        assert types == [p[1] for p in PARAMS[name]], (name, types)
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    m = re.search(r"pub fn render_probes\(&self, ([^)]*)\) -> Vec<\[\[f32; 3\]; 9\]>", wrapper)
    assert m and [a.split(":")[0].strip() for a in m.group(1).split(",")] == ["points", "rows_per_pixel", "seed"]
    call = re.search(r"mi_rt::mi_render_probes\(([^;]*)\)\s*\n", wrapper).group(1)
    assert len(call.split(",")) == len(PARAMS["mi_render_probes"])
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert re.search(r"std::vector<float> render_probes\(const std::vector<float>& points, uint32_t rows_per_pixel", hpp)
    call = re.search(r"return mi_render_probes\(([^;]*)\);", hpp).group(1)
    assert len(call.split(",")) == len(PARAMS["mi_render_probes"])
    src = tmp_path / "hp.cpp"
    src.write_text('#include "tracing.hpp"\nusing namespace cs397;\n'
                   "std::vector<float> (Scene::*probes)(const std::vector<float>&, uint32_t, uint32_t, int, mi_stats*, RgbImage*,\n"
                   "                                    std::vector<float>*) const = &Scene::render_probes;\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "cs397raytracingsp22_amd", "host"), str(src)], check=True)
    import cs397raytracingsp22_amd as pkg
    for cls, names in ((pkg.Context, ("render_probes", "render_probes_device")), (pkg.Scene, ("render_probes",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    for helper in ("check_probe_table", "probe_grid", "sh9_basis", "sh9_irradiance"):
        assert callable(getattr(pkg, helper)), helper
