"""Hemisphere occlusion (mi_hemisphere_occlusion / mi_hemisphere_occlusion_device): what can be checked without a GPU — the header as
C99, the ctypes mirror, the names in the Rust, C++ and Python mirrors, and the Python input checking of points, normals, sample
counts and flags."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_hemisphere_occlusion", "mi_hemisphere_occlusion_device"]
ARITY = {"mi_hemisphere_occlusion": 13, "mi_hemisphere_occlusion_device": 14}
INF = float("inf")


def test_header_declares_both_and_compiles_as_c99(tmp_path):
    src = tmp_path / "hemi.c"
    args = "mi_ctx*, uint32_t, const float*, const float*, uint32_t, uint32_t, float, float, uint32_t, uint32_t, uint32_t, uint32_t*, float*"
    src.write_text('#include "mi_rt.h"\n'
                   "int main(void) {\n"
                   f"    int (*host)({args}) = mi_hemisphere_occlusion;\n"
                   f"    int (*dev)({args}, void*) = mi_hemisphere_occlusion_device;\n"
                   "    uint32_t flag = MI_HEMI_WORLD_RADIUS;\n"
                   "    return host == 0 || dev == 0 || flag != 1u;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "hemi.o")],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "mi_rt.h")).read()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)          # additive: the version did not move
    assert re.search(r"#define\s+MI_HEMI_WORLD_RADIUS\s+1u\b", hdr)
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code).group(1)
        assert len(args.split(",")) == ARITY[name], name
    # what the header has to say about them: the keying, the unnormalised normal and direction, the two ways to split a bake
    doc = " ".join(hdr.split())
    for phrase in ("(seed, first_key + i, 2s)", "(seed, first_key + i, 2s + 1)", "NOT normalised", "first_sample advanced",
                   "first_key advanced", "UNSPECIFIED count"):
        assert phrase in doc, phrase


def test_ctypes_mirror_exposes_both():
    from cs397raytracingsp22_amd import abi
    lib = abi.load()
    C = abi.C
    want = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
            C.c_uint32, C.c_void_p, C.c_void_p]
    for name in NAMES:
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == ARITY[name], name
        assert fn.restype is C.c_int
        assert list(fn.argtypes[:13]) == want, name
    assert lib.mi_hemisphere_occlusion_device.argtypes[13] is C.c_void_p
    assert abi.MI_HEMI_WORLD_RADIUS == 1 and abi.MI_RT_ABI_VERSION == 5


def test_rust_cpp_and_python_mirrors_name_them():
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        assert re.search(rf"pub\s+fn\s+{name}\s*\(", block), name
    assert "pub const MI_HEMI_WORLD_RADIUS: u32 = 1;" in rust
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn hemisphere_occlusion(" in wrapper and "mi_rt::mi_hemisphere_occlusion(" in wrapper
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "hemisphere_occlusion(" in hpp and "mi_hemisphere_occlusion(" in hpp
    py = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "tracing.py")).read()
    for name in NAMES:
        assert f"self._lib.{name}(" in py, name
    from cs397raytracingsp22_amd import Context, Scene
    for cls, names in ((Context, ("hemisphere_occlusion", "hemisphere_occlusion_device")), (Scene, ("ambient_occlusion",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_checker_accepts():
    from cs397raytracingsp22_amd import abi
    from cs397raytracingsp22_amd.tracing import check_hemisphere
    p, n, ns, t_min, t_max, flags, first = check_hemisphere([[0, 0, 0], [1, 2, 3]], [[0, 1, 0], [0, 0, 2]], 64)     # lists
    assert p.dtype == np.float32 and n.dtype == np.float32 and p.shape == n.shape == (2, 3)
    assert p.flags["C_CONTIGUOUS"] and n.flags["C_CONTIGUOUS"]
    assert (ns, t_min, t_max, flags, first) == (64, 0.001, INF, 0, 0)
    assert n[1].tolist() == [0.0, 0.0, 2.0]                               # the normal is not normalised
    exact = np.array([[1.0, np.nextafter(np.float32(1.0), np.float32(0.0)), -0.0]], np.float32)
    p, n, *_ = check_hemisphere(exact, exact, 1)
    assert p.tobytes() == exact.tobytes() and n.tobytes() == exact.tobytes()     # float32 goes through bit for bit
    p, n, *_ = check_hemisphere(np.zeros((4, 3), np.float64), np.ones((4, 3), np.float64), 65535, 0.0, 2.5, abi.MI_HEMI_WORLD_RADIUS)
    assert p.dtype == np.float32 and len(p) == 4
    strided = np.arange(24, dtype=np.float32).reshape(4, 6)[:, ::2]
    p, *_ = check_hemisphere(strided, strided, 3)
    assert p.flags["C_CONTIGUOUS"] and p[1].tolist() == [6.0, 8.0, 10.0]
    p, n, *_ = check_hemisphere(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 8)
    assert p.shape == (0, 3)
    assert check_hemisphere(exact, exact, 1, first_sample=(1 << 31) - 1)[6] == (1 << 31) - 1     # first_sample + n_samples == 2^31 is legal
    nan_point = np.array([[np.nan, 0, 0]], np.float32)
    check_hemisphere(nan_point, exact, 4)                                 # a bad point is the library's business (unspecified count)


def test_checker_refuses():
    from cs397raytracingsp22_amd.tracing import check_hemisphere
    ok = np.zeros((4, 3), np.float32)
    for pts, nrm in ((np.zeros((4, 2), np.float32), ok), (ok, np.zeros((4, 4), np.float32)), (np.zeros(12, np.float32), ok),
                     (ok, np.zeros((3, 3), np.float32)), (np.zeros((5, 3), np.float32), ok), (np.zeros((2, 2, 3), np.float32), ok),
                     (np.float32(1.0), ok)):
        with pytest.raises(ValueError):
            check_hemisphere(pts, nrm, 16)
    for n_samples in (0, 65536, -1):
        with pytest.raises(ValueError):
            check_hemisphere(ok, ok, n_samples)
    for flags in (2, 3, 0x80000000):                                      # an unknown flag bit
        with pytest.raises(ValueError):
            check_hemisphere(ok, ok, 16, flags=flags)
    with pytest.raises(ValueError):
        check_hemisphere(ok, ok, 2, first_sample=(1 << 31) - 1)           # first_sample + n_samples > 2^31
    with pytest.raises(ValueError):
        check_hemisphere(ok, ok, 16, t_min=float("nan"))
    with pytest.raises(ValueError):
        check_hemisphere(ok, ok, 16, t_max=float("nan"))
    with pytest.raises((ValueError, TypeError)):
        check_hemisphere(np.array([["a", "b", "c"]]), np.zeros((1, 3), np.float32), 16)


def test_scene_ambient_occlusion_checks_its_input_before_it_touches_a_device():
    from cs397raytracingsp22_amd import scenes
    sc = scenes.config1(8, 8, 1, 2)
    ok = np.zeros((4, 3), np.float32)
    for kw in (dict(points=np.zeros((4, 2), np.float32), normals=ok), dict(points=ok, normals=ok[:3]), dict(points=ok, normals=ok, samples=0),
               dict(points=ok, normals=ok, samples=65536), dict(points=ok, normals=ok, radius=float("nan"))):
        with pytest.raises(ValueError):
            sc.ambient_occlusion(**kw)
