"""Ray queries (mi_intersect_rays / mi_shade_rays and their _device forms): what can be checked without a GPU — the Python input
checking, the header as C99, the ctypes mirror's arity, and the names in the Rust and C++ mirrors."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_intersect_rays", "mi_intersect_rays_device", "mi_shade_rays", "mi_shade_rays_device"]
ARITY = {"mi_intersect_rays": 15, "mi_intersect_rays_device": 16, "mi_shade_rays": 8, "mi_shade_rays_device": 9}


def test_check_rays_accepts_lists_and_float64():
    from cs397raytracingsp22_amd.tracing import check_rays
    o, d, t_min, t_max = check_rays([[0, 0, 0], [1, 2, 3]], np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0]], np.float64))
    for a in (o, d):
        assert a.dtype == np.float32 and a.shape == (2, 3) and a.flags["C_CONTIGUOUS"]
    assert t_min == pytest.approx(0.001) and t_max == float("inf")
    # a strided view comes back contiguous, directions are not normalised
    big = np.arange(24, dtype=np.float64).reshape(4, 6)
    o, d, _, _ = check_rays(big[:, 0:3], big[:, 3:6] * 10.0, 0.0, 5.0)
    assert o.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"] and d[1, 2] == np.float32(110.0)
    o, d, _, _ = check_rays(np.zeros((0, 3)), np.zeros((0, 3)))
    assert o.shape == (0, 3) and d.shape == (0, 3)


def test_check_rays_rejects_bad_input():
    from cs397raytracingsp22_amd.tracing import check_rays
    ok = np.zeros((4, 3))
    with pytest.raises(ValueError):
        check_rays(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        check_rays(ok, np.zeros((4, 2)))
    with pytest.raises(ValueError):
        check_rays(np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError):
        check_rays(ok, np.zeros((5, 3)))
    with pytest.raises(ValueError):
        check_rays(ok, ok, t_min=float("nan"))
    with pytest.raises(ValueError):
        check_rays(ok, ok, t_max=float("nan"))
    check_rays(ok, ok, t_min=0.0, t_max=float("inf"))          # +inf is legal


def test_header_compiles_as_c99_and_declares_the_four(tmp_path):
    src = tmp_path / "rq.c"
    src.write_text('#include "mi_rt.h"\n'
                   "typedef void (*fn)(void);\n"
                   "int main(void) {\n"
                   "    fn f[4] = { (fn)mi_intersect_rays, (fn)mi_intersect_rays_device, (fn)mi_shade_rays, (fn)mi_shade_rays_device };\n"
                   "    return f[0] == 0 || f[1] == 0 || f[2] == 0 || f[3] == 0;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "rq.o")],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "mi_rt.h")).read()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)          # additive: the version did not move
    assert ">= 96 small triangles" in hdr and ">= 32 small triangles" not in hdr


def test_ctypes_mirror_exposes_them_with_the_right_arity():
    from cs397raytracingsp22_amd import abi
    lib = abi.load()
    for name in NAMES:
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == ARITY[name], name
        assert fn.restype is abi.C.c_int
    # the header's own argument counts
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_rt.h")).read(), flags=re.S)
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", hdr).group(1)
        assert len(args.split(",")) == ARITY[name], name


def test_rust_and_cpp_mirrors_name_them():
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        assert re.search(rf"pub\s+fn\s+{name}\s*\(", block), name
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn intersect_rays(" in wrapper and "pub fn shade_rays(" in wrapper
    assert "mi_rt::mi_intersect_rays(" in wrapper and "mi_rt::mi_shade_rays(" in wrapper
    assert "#[repr(C)]" not in wrapper
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "intersect_rays(" in hpp and "shade_rays(" in hpp and "mi_intersect_rays(" in hpp and "mi_shade_rays(" in hpp
    # the device forms are reachable from Python (Context) and declared for C++ through the header tracing.hpp includes
    py = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "tracing.py")).read()
    for name in NAMES:
        assert f"self._lib.{name}(" in py, name


def test_scene_and_context_have_the_methods():
    from cs397raytracingsp22_amd import Context, Scene
    for cls, names in ((Context, ("intersect_rays", "intersect_rays_device", "shade_rays", "shade_rays_device")), (Scene, ("intersect_rays", "shade_rays"))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
