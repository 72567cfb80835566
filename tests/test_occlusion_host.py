"""Occlusion queries (mi_occluded_rays / mi_occluded_rays_device): what can be checked without a GPU — the header as C99, the ctypes
mirror, the names in the Rust and C++ mirrors, and the Python input checking of the per-ray `ray_t_max`."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_occluded_rays", "mi_occluded_rays_device"]
ARITY = {"mi_occluded_rays": 10, "mi_occluded_rays_device": 11}
INF = float("inf")


def test_header_declares_both_and_compiles_as_c99(tmp_path):
    src = tmp_path / "occ.c"
    src.write_text('#include "mi_rt.h"\n'
                   "int main(void) {\n"
                   "    int (*host)(mi_ctx*, uint32_t, const float*, const float*, float, float, const float*, uint32_t, uint32_t, uint8_t*) = mi_occluded_rays;\n"
                   "    int (*dev)(mi_ctx*, uint32_t, const float*, const float*, float, float, const float*, uint32_t, uint32_t, uint8_t*, void*) = mi_occluded_rays_device;\n"
                   "    return host == 0 || dev == 0;\n"
                   "}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "occ.o")],
                   check=True)
    hdr = open(os.path.join(ROOT, "include", "mi_rt.h")).read()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)          # additive: the version did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        args = re.search(rf"\b{name}\s*\(([^)]*)\)\s*;", code).group(1)
        assert len(args.split(",")) == ARITY[name], name
    # what the header has to say about them
    doc = " ".join(hdr.split())
    assert "UNSPECIFIED answer" in doc and "[eps, 1 - eps]" in doc and "NOT normalised" in doc


def test_ctypes_mirror_exposes_both():
    from cs397raytracingsp22_amd import abi
    lib = abi.load()
    for name in NAMES:
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert len(fn.argtypes) == ARITY[name], name
        assert fn.restype is abi.C.c_int
        assert fn.argtypes[4] is abi.C.c_float and fn.argtypes[5] is abi.C.c_float and fn.argtypes[7] is abi.C.c_uint32


def test_rust_and_cpp_mirrors_name_them():
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        assert re.search(rf"pub\s+fn\s+{name}\s*\(", block), name
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn occluded_rays(" in wrapper and "mi_rt::mi_occluded_rays(" in wrapper
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "occluded_rays(" in hpp and "mi_occluded_rays(" in hpp
    py = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "tracing.py")).read()
    for name in NAMES:
        assert f"self._lib.{name}(" in py, name
    from cs397raytracingsp22_amd import Context, Scene
    for cls, names in ((Context, ("occluded_rays", "occluded_rays_device")), (Scene, ("occluded_rays",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_ray_t_max_checker_accepts():
    from cs397raytracingsp22_amd.tracing import check_ray_t_max
    assert check_ray_t_max(None, 5) is None
    t = check_ray_t_max([1.0, 2.5, INF], 3)                              # a list; +inf is legal
    assert t.dtype == np.float32 and t.shape == (3,) and t.flags["C_CONTIGUOUS"] and t[2] == np.float32(INF)
    t = check_ray_t_max(np.array([0.25, 1e300, -1.0], np.float64), 3)    # float64 is converted (1e300 -> +inf)
    assert t.dtype == np.float32 and t[0] == np.float32(0.25) and np.isinf(t[1]) and t[2] == np.float32(-1.0)
    t = check_ray_t_max(np.array([3, 4], np.int64), 2)                   # whole numbers too
    assert t.dtype == np.float32 and t.tolist() == [3.0, 4.0]
    strided = np.arange(8, dtype=np.float32)[::2]
    t = check_ray_t_max(strided, 4)
    assert t.flags["C_CONTIGUOUS"] and t.tolist() == [0.0, 2.0, 4.0, 6.0]
    exact = np.array([1.0, np.nextafter(np.float32(1.0), np.float32(0.0))], np.float32)
    assert check_ray_t_max(exact, 2).tobytes() == exact.tobytes()        # float32 goes through bit for bit
    assert check_ray_t_max(np.zeros(0, np.float32), 0).shape == (0,)
    assert check_ray_t_max(np.full(4, INF, np.float32), 4).shape == (4,)


def test_ray_t_max_checker_refuses():
    from cs397raytracingsp22_amd.tracing import check_ray_t_max
    for bad, n in ((np.zeros(3, np.float32), 4),                         # wrong length
                   (np.zeros(5, np.float32), 4),
                   (np.zeros((4, 1), np.float32), 4),                    # wrong dimension
                   (np.float32(1.0), 1),                                 # a scalar is not [n]
                   (np.zeros((2, 2), np.float32), 4),
                   (np.zeros(4, np.complex64), 4),                       # wrong dtype
                   (np.zeros(4, bool), 4),
                   (np.array(["1", "2", "3", "4"]), 4),
                   (np.array([1.0, None, 2.0, 3.0], object), 4),
                   (np.array([1.0, float("nan"), 2.0, 3.0], np.float32), 4),   # NaN
                   ([float("nan")], 1)):
        with pytest.raises(ValueError):
            check_ray_t_max(bad, n)


def test_check_rays_is_unchanged_for_existing_callers():
    from cs397raytracingsp22_amd.tracing import check_rays
    out = check_rays(np.zeros((2, 3)), np.ones((2, 3)), 0.0, 5.0)
    assert len(out) == 4 and out[2] == 0.0 and out[3] == 5.0
    with pytest.raises(TypeError):
        check_rays(np.zeros((2, 3)), np.ones((2, 3)), 0.0, 5.0, None)    # no fifth argument crept in
