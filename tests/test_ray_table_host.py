"""Ray-table rendering (mi_render_rays / mi_render_rays_device): what can be checked without a GPU — the two prototypes in the header,
the ctypes mirror and the Rust text with identical parameter lists, the Python input checking (check_ray_table), the panorama helper
(equirect_ray_table), and the symbols of the library as built."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_render_rays", "mi_render_rays_device"]
# the parameter lists, written once: (C type, Rust type, ctypes type name)
VP = ("void*", "*mut c_void", "c_void_p")
U32 = ("uint32_t", "u32", "c_uint32")
TABLE = [("const float*", "*const f32", "c_void_p"), ("const float*", "*const f32", "c_void_p"), U32]
HEAD = [("mi_ctx*", "*mut mi_ctx", "c_void_p"), ("const mi_camera_desc*", "*const mi_camera_desc", "LP_mi_camera_desc"),
        ("const mi_render_opts*", "*const mi_render_opts", "LP_mi_render_opts")]
STATS = ("mi_stats*", "*mut mi_stats", "LP_mi_stats")
PARAMS = {
    "mi_render_rays": HEAD + TABLE + [("float*", "*mut f32", "c_void_p"), ("uint8_t*", "*mut u8", "c_void_p"),
                                      ("uint32_t*", "*mut u32", "c_void_p"), STATS],
    "mi_render_rays_device": HEAD + TABLE + [U32, U32, VP, VP, VP, VP, STATS],
}


def _header():
    return open(os.path.join(ROOT, "include", "mi_rt.h")).read()


def test_header_declares_both_with_the_stated_parameter_lists(tmp_path):
    hdr = _header()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)           # additive: the version did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        args = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code).group(1)
        types = [" ".join(re.match(r"(.+?)\s*\w+$", " ".join(a.split())).group(1).split()) for a in args.split(",")]
        assert types == [p[0] for p in PARAMS[name]], (name, types)
    # and as C99, through function pointers of exactly these types
    src = tmp_path / "rt.c"
    src.write_text('#include "mi_rt.h"\nint main(void) {\n' + "".join(
        f"    int (*f{k})({', '.join(p[0] for p in PARAMS[n])}) = {n};\n" for k, n in enumerate(NAMES)) + "    return f0 == 0 || f1 == 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "rt.o")],
                   check=True)
    doc = " ".join(hdr.split())
    for phrase in ("[rays_per_pixel][H][W][3]", "((s*H + y)*W + x)*3", "(seed, y*W + x, s)", "NOT normalised", "need NOT be a perfect square",
                   "MI_ERR_UNSUPPORTED", "MI_ERR_NO_SCENE", "MI_OPT_NO_TILE_MASKS", "MI_ERR_OOM"):
        assert phrase in doc, phrase


def test_ctypes_mirror_has_the_same_parameter_lists():
    from cs397raytracingsp22_amd import abi
    lib = abi.load()
    for name in NAMES:
        assert name in abi.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == len(PARAMS[name]), name
        for k, (t, p) in enumerate(zip(fn.argtypes, PARAMS[name])):             # c_uint32 is an alias: compare the types, not their names
            assert (t is getattr(C, p[2])) if hasattr(C, p[2]) else (t.__name__ == p[2]), (name, k, t, p[2])


def test_rust_text_has_the_same_parameter_lists():
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    for name in NAMES:
        args = re.search(rf"pub\s+fn\s+{name}\s*\(([^)]*)\)\s*->\s*c_int;", block).group(1)
        types = [" ".join(a.split(":", 1)[1].split()) for a in args.split(",")]
        assert types == [p[1] for p in PARAMS[name]], (name, types)
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn render_rays(" in wrapper and "mi_rt::mi_render_rays(" in wrapper
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "render_rays(" in hpp and "mi_render_rays(" in hpp
    from cs397raytracingsp22_amd import Context, Scene
    for cls, names in ((Context, ("render_rays", "render_rays_device")), (Scene, ("render_rays",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)


def test_both_symbols_resolve_from_the_library_as_built():
    from cs397raytracingsp22_amd import abi
    raw = C.CDLL(abi.LIB_PATH)                            # a fresh handle: no prototypes of the mirror involved
    for name in NAMES:
        assert C.cast(getattr(raw, name), C.c_void_p).value
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NAMES:
        assert re.search(rf"\bT {name}$", out, flags=re.M), name


# ---------------------------------------------------------------- check_ray_table
def _cam(**kw):
    from cs397raytracingsp22_amd import Camera
    base = dict(screen_width=7, screen_height=5, aa_sample_count=4, path_depth=6)
    base.update(kw)
    return Camera(**base)


def _table(s, h=5, w=7, dtype=np.float32):
    o = np.zeros((s, h, w, 3) if s else (h, w, 3), dtype)
    d = np.ones_like(o)
    return o, d


def test_check_ray_table_accepts():
    from cs397raytracingsp22_amd.tracing import check_ray_table
    cam = _cam()
    for s, rows in ((4, 4), (1, 1), (0, 1)):                                  # [aa, H, W, 3], [1, H, W, 3], [H, W, 3]
        o, d, r = check_ray_table(cam, *_table(s))
        assert r == rows and o.shape == d.shape == (rows, 5, 7, 3)
        assert o.dtype == d.dtype == np.float32 and o.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"]
    big = np.arange(4 * 5 * 14 * 3, dtype=np.float32).reshape(4, 5, 14, 3)
    o, d, _ = check_ray_table(cam, big[:, :, ::2], big[:, :, 1::2])           # strided views are made contiguous, values kept
    assert o.flags["C_CONTIGUOUS"] and np.array_equal(o, big[:, :, ::2]) and np.array_equal(d, big[:, :, 1::2])
    # a non-square aa_sample_count: the square exists for generate_rays' jitter grid only
    for aa in (3, 5, 7, 65535):
        assert check_ray_table(_cam(aa_sample_count=aa), *_table(1))[2] == 1
    assert check_ray_table(_cam(aa_sample_count=3), *_table(3))[2] == 3
    # the pose, projection and lens fields are ignored: anything goes, non-finite values included
    nan, inf = float("nan"), float("inf")
    odd = _cam(eyepoint=(nan, inf, -inf), view_dir=(0.0, 0.0, 0.0), up=(nan, nan, nan), projection_mode=77, focal_length=nan,
               focus_dist=-inf, lens_radius=nan)
    assert check_ray_table(odd, *_table(4))[2] == 4
    assert check_ray_table(_cam(max_trace_dist=inf), *_table(1))[2] == 1      # +inf is legal, as in mi_render
    assert check_ray_table(_cam(path_depth=0), *_table(1))[2] == 1
    # non-finite rays are not refused
    o, d = _table(1)
    d[0, 0, 0] = (nan, 0.0, inf)
    o[0, 1, 1] = (inf, nan, 0.0)
    assert check_ray_table(cam, o, d)[2] == 1


def test_check_ray_table_refuses():
    from cs397raytracingsp22_amd.tracing import ShadingMode, check_ray_table
    cam = _cam()
    o4, d4 = _table(4)
    bad_tables = [
        (np.zeros((4, 5, 7), np.float32), np.zeros((4, 5, 7), np.float32)),           # no xyz axis
        (np.zeros((4, 5, 7, 2), np.float32), np.zeros((4, 5, 7, 2), np.float32)),     # two components
        (np.zeros((4, 7, 5, 3), np.float32), np.zeros((4, 7, 5, 3), np.float32)),     # W and H swapped
        (np.zeros((4 * 5 * 7, 3), np.float32), np.zeros((4 * 5 * 7, 3), np.float32)), # flat [n, 3]
        (np.zeros((1, 4, 5, 7, 3), np.float32), np.zeros((1, 4, 5, 7, 3), np.float32)),
        (o4, d4[:1]),                                                                 # origins and dirs differ in rows
        (o4[0], d4),
        _table(2), _table(3), _table(5), _table(16),                                  # S not in {1, aa}
        _table(4, dtype=np.float64), (o4, d4.astype(np.float16)), _table(4, dtype=np.int32),      # dtype
        (o4.tolist(), d4),                                                            # a list is float64
    ]
    for o, d in bad_tables:
        with pytest.raises(ValueError):
            check_ray_table(cam, o, d)
    nan = float("nan")
    for kw in (dict(path_samples=2), dict(path_samples=0), dict(shading_mode=ShadingMode.Phong), dict(shading_mode=5),
               dict(max_trace_dist=nan), dict(gamma=0.0), dict(gamma=-1.0), dict(gamma=nan), dict(gamma=float("inf")),
               dict(aa_sample_count=0), dict(aa_sample_count=65536), dict(screen_width=0), dict(screen_height=40000),
               dict(path_depth=65536)):
        with pytest.raises(ValueError):
            check_ray_table(_cam(**kw), *_table(1))
    with pytest.raises(ValueError, match="shade_rays"):                               # the message points to the call that does it
        check_ray_table(_cam(path_samples=2), o4, d4)


def test_render_rays_refuses_before_any_library_call():
    """Context.render_rays checks first: a bad table raises ValueError even on an object that has no context at all."""
    from cs397raytracingsp22_amd import Context, Scene
    ctx = Context.__new__(Context)                        # no mi_ctx_create: any library call would fail on the missing handle
    with pytest.raises(ValueError):
        Context.render_rays(ctx, _cam(), *_table(2))
    with pytest.raises(ValueError):
        Scene(_cam(path_samples=2), []).render_rays(*_table(4))


# ---------------------------------------------------------------- equirect_ray_table
def test_equirect_table_shapes_unit_directions_and_seed():
    from cs397raytracingsp22_amd.tracing import check_ray_table, equirect_ray_table
    eye = (0.25, 1.5, -2.0)
    o, d = equirect_ray_table(75, 41, eye, samples=4, seed=9)
    assert o.shape == d.shape == (4, 41, 75, 3) and o.dtype == d.dtype == np.float32
    assert np.array_equal(o, np.broadcast_to(np.asarray(eye, np.float32), o.shape))
    norm = np.sqrt((d.astype(np.float64) ** 2).sum(axis=-1))
    assert float(np.abs(norm - 1.0).max()) <= 2e-7                            # f32 rounding of a unit f64 vector
    o2, d2 = equirect_ray_table(75, 41, eye, samples=4, seed=9)
    assert o2.tobytes() == o.tobytes() and d2.tobytes() == d.tobytes()        # same seed, same table
    _, d3 = equirect_ray_table(75, 41, eye, samples=4, seed=10)
    assert d3.tobytes() != d.tobytes()
    assert len({d[s].tobytes() for s in range(4)}) == 4                       # the samples of a pixel are jittered apart
    # every sample stays inside its own pixel's footprint of the panorama
    lon = np.arctan2(d[..., 0].astype(np.float64), -d[..., 2].astype(np.float64))
    lat = np.arcsin(np.clip(d[..., 1].astype(np.float64), -1.0, 1.0))
    x = (lon / (2 * np.pi) + 0.5) * 75 - np.arange(75)[None, None, :]
    y = (0.5 - lat / np.pi) * 41 - np.arange(41)[None, :, None]
    assert x.min() > -1e-4 and x.max() < 1 + 1e-4 and y.min() > -1e-4 and y.max() < 1 + 1e-4
    check_ray_table(_cam(screen_width=75, screen_height=41, aa_sample_count=4), o, d)
    # one sample: pixel centres, whatever the seed
    _, c1 = equirect_ray_table(8, 4, eye, samples=1, seed=1)
    _, c2 = equirect_ray_table(8, 4, eye, samples=1, seed=2)
    assert c1.shape == (1, 4, 8, 3) and c1.tobytes() == c2.tobytes()
    for bad in ((0, 4, 1), (8, 0, 1), (8, 4, 0)):
        with pytest.raises(ValueError):
            equirect_ray_table(bad[0], bad[1], eye, samples=bad[2])


def test_equirect_poles_and_seam_are_axis_aligned():
    from cs397raytracingsp22_amd.tracing import equirect_dirs, equirect_ray_table
    pi = np.pi
    lon = np.array([0.0, 0.5 * pi, -0.5 * pi, pi, -pi, 0.3, 0.3])
    lat = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.5 * pi, -0.5 * pi])
    d = equirect_dirs(lon, lat)
    want = np.array([[0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 0, 1], [0, 0, 1], [0, 1, 0], [0, -1, 0]], np.float32)
    assert d.dtype == np.float32 and d.tobytes() == want.tobytes()            # exact, and no negative zero
    # in a table: an odd-sized panorama looks straight down -z through its centre pixel; a width that is 2 mod 4 puts pixel centres on
    # +-x; the first column's left edge is the seam (+z), met by no centre
    _, t = equirect_ray_table(75, 41, (0, 0, 0))
    assert t[0, 20, 37].tobytes() == np.array([0, 0, -1], np.float32).tobytes()
    _, t = equirect_ray_table(6, 3, (0, 0, 0))
    assert t[0, 1, 4].tobytes() == np.array([1, 0, 0], np.float32).tobytes()      # (4.5 / 6 - 0.5) * 2 pi = +pi / 2
    assert t[0, 1, 1].tobytes() == np.array([-1, 0, 0], np.float32).tobytes()
    assert np.all(t[0, 0, :, 1] > 0) and np.all(t[0, 2, :, 1] < 0) and np.all(t[0, 1, :, 1] == 0)
    assert t[0, 1, 0, 2] > 0 and t[0, 1, 5, 2] > 0                                # the outer columns look towards the seam
