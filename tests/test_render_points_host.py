"""Point-table rendering (mi_render_points / mi_render_points_device): what can be checked without a GPU — the two prototypes in the
header, the ctypes mirror, the C++ mirror and the Rust text with identical parameter lists, the Python input checking
(check_point_table) and the host helper that makes a mesh's point table (lightmap_texels), whose row flip is pinned against the
oracle's own texture sampler."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_render_points", "mi_render_points_device"]
# the parameter lists, written once: (C type, Rust type, ctypes type name)
VP = ("void*", "*mut c_void", "c_void_p")
U32 = ("uint32_t", "u32", "c_uint32")
TABLE = [("const float*", "*const f32", "c_void_p"), ("const float*", "*const f32", "c_void_p"), U32]
HEAD = [("mi_ctx*", "*mut mi_ctx", "c_void_p"), ("const mi_camera_desc*", "*const mi_camera_desc", "LP_mi_camera_desc"),
        ("const mi_render_opts*", "*const mi_render_opts", "LP_mi_render_opts")]
STATS = ("mi_stats*", "*mut mi_stats", "LP_mi_stats")
PARAMS = {
    "mi_render_points": HEAD + TABLE + [("float*", "*mut f32", "c_void_p"), ("uint8_t*", "*mut u8", "c_void_p"),
                                        ("uint32_t*", "*mut u32", "c_void_p"), STATS],
    "mi_render_points_device": HEAD + TABLE + [U32, U32, VP, VP, VP, VP, STATS],
}


def _header():
    return open(os.path.join(ROOT, "include", "mi_rt.h")).read()


def _c_types(args):
    return [" ".join(re.match(r"(.+?)\s*\w+$", " ".join(a.split())).group(1).split()) for a in args.split(",")]


def test_header_declares_both_with_the_stated_parameter_lists(tmp_path):
    hdr = _header()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr)           # additive: the version did not move
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NAMES:
        args = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code).group(1)
        assert _c_types(args) == [p[0] for p in PARAMS[name]], name
        # the contract is mi_render_rays': the same argument types, one for one
        rays = re.search(rf"\bint\s+{name.replace('points', 'rays')}\s*\(([^)]*)\)\s*;", code).group(1)
        assert _c_types(args) == _c_types(rays), name
    src = tmp_path / "pt.c"
    src.write_text('#include "mi_rt.h"\nint main(void) {\n' + "".join(
        f"    int (*f{k})({', '.join(p[0] for p in PARAMS[n])}) = {n};\n" for k, n in enumerate(NAMES)) + "    return f0 == 0 || f1 == 0;\n}\n")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "pt.o")],
                   check=True)
    # what the comment has to state: the two streams, the empty-texel rule, the origin as given, t_min in units of |d|, the equivalence
    # with mi_render_rays, non-finite texels
    doc = " ".join(re.sub(r"\n \*", "\n", hdr[hdr.index("point-table rendering"):hdr.index("int  mi_render_points(")]).split())
    for phrase in ("[rows_per_pixel][H][W][3]", "(seed, W*H + y*W + x, s)", "(seed, y*W + x, s)", "all zero", "either sign of zero",
                   "used as given", "t_min = 0.001", "|d| <= 1", "mi_render_points(points, normals) == mi_render_rays(points, d)",
                   "never faults", "that pixel only", "NOT normalised", "empty texels included"):
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
    m = re.search(r"pub fn render_points\(&self, ([^)]*)\) -> RgbImage", wrapper)
    assert m and [a.split(":")[0].strip() for a in m.group(1).split(",")] == ["points", "normals", "rows_per_pixel", "seed"]
    call = re.search(r"mi_rt::mi_render_points\(([^;]*)\)\s*\n", wrapper).group(1)
    assert len(call.split(",")) == len(PARAMS["mi_render_points"])
    # the C++ mirror: Scene::render_points exists and compiles against the header's prototype (the header is what it includes)
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert re.search(r"RgbImage render_points\(const std::vector<float>& points, const std::vector<float>& normals, uint32_t rows_per_pixel", hpp)
    call = re.search(r"return mi_render_points\(([^;]*)\);", hpp).group(1)
    assert len(call.split(",")) == len(PARAMS["mi_render_points"])
    src = tmp_path / "hp.cpp"
    src.write_text('#include "tracing.hpp"\nusing namespace cs397;\n'
                   "RgbImage (Scene::*bake)(const std::vector<float>&, const std::vector<float>&, uint32_t, uint32_t, int, mi_stats*,\n"
                   "                        std::vector<float>*) const = &Scene::render_points;\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "cs397raytracingsp22_amd", "host"), str(src)], check=True)
    import cs397raytracingsp22_amd as pkg
    for cls, names in ((pkg.Context, ("render_points", "render_points_device")), (pkg.Scene, ("render_points",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert callable(pkg.check_point_table) and callable(pkg.lightmap_texels)


# ---------------------------------------------------------------- check_point_table
def _cam(**kw):
    from cs397raytracingsp22_amd import Camera
    base = dict(screen_width=7, screen_height=5, aa_sample_count=4, path_depth=6)
    base.update(kw)
    return Camera(**base)


def _table(s, h=5, w=7, dtype=np.float32):
    p = np.zeros((s, h, w, 3) if s else (h, w, 3), dtype)
    n = np.ones_like(p)
    return p, n


def test_check_point_table_accepts():
    from cs397raytracingsp22_amd.tracing import check_point_table
    cam = _cam()
    for s, rows in ((0, 1), (4, 4), (1, 1)):                                  # [H, W, 3], [aa, H, W, 3], [1, H, W, 3]
        p, n, r = check_point_table(cam, *_table(s))
        assert r == rows and p.shape == n.shape == (rows, 5, 7, 3)
        assert p.dtype == n.dtype == np.float32 and p.flags["C_CONTIGUOUS"] and n.flags["C_CONTIGUOUS"]
    assert check_point_table(_cam(aa_sample_count=3), *_table(3))[2] == 3     # a non-square aa is fine ...
    assert check_point_table(_cam(aa_sample_count=7), *_table(0))[2] == 1
    nan = float("nan")
    assert check_point_table(_cam(eyepoint=(nan, nan, nan)), *_table(4))[2] == 4      # ... and so is a NaN eyepoint: the pose is ignored
    p, n = _table(0)
    n[2, 3] = 0.0                                                             # an empty texel and a non-finite one are not the checker's business
    p[1, 1] = (nan, 0.0, float("inf"))
    assert check_point_table(cam, p, n)[2] == 1


def test_check_point_table_refuses():
    from cs397raytracingsp22_amd.tracing import ShadingMode, check_point_table
    cam = _cam()
    p4, n4 = _table(4)
    for p, n in (_table(4, dtype=np.float64),                                 # float64
                 _table(4, h=7, w=5), _table(0, h=5, w=8), _table(0, h=4, w=7),       # wrong H / W
                 _table(2),                                                   # 2 rows when aa = 4
                 (p4, n4[:1]), (p4[0], n4)):                                  # differing shapes
        with pytest.raises(ValueError):
            check_point_table(cam, p, n)
    for kw in (dict(path_samples=2), dict(shading_mode=ShadingMode.Phong), dict(max_trace_dist=float("nan")), dict(gamma=0.0)):
        with pytest.raises(ValueError):
            check_point_table(_cam(**kw), *_table(0))
    with pytest.raises(ValueError, match="points must be float32"):           # the messages name this call's arguments
        check_point_table(cam, p4.astype(np.float64), n4)
    with pytest.raises(ValueError, match="a point table holds 1 row or aa_sample_count = 4 rows"):
        check_point_table(cam, *_table(2))


def test_render_points_refuses_before_any_library_call():
    from cs397raytracingsp22_amd import Context, Scene
    ctx = Context.__new__(Context)                        # no mi_ctx_create: any library call would fail on the missing handle
    with pytest.raises(ValueError):
        Context.render_points(ctx, _cam(), *_table(2))
    with pytest.raises(ValueError):
        Scene(_cam(path_samples=2), []).render_points(*_table(4))


# ---------------------------------------------------------------- lightmap_texels
QUAD_P = np.float32([[-1, 0, 1], [1, 0, 1], [1, 0, -1], [-1, 0, -1]])          # uv (0,0) (1,0) (1,1) (0,1): x = 2u - 1, z = 1 - 2v
QUAD_N = np.float32([[0, 1, 0]] * 4)
QUAD_T = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]])
QUAD_I = np.uint32([[0, 1, 2], [0, 2, 3]])


def test_lightmap_texels_quad():
    from cs397raytracingsp22_amd import lightmap_texels
    pts, nrm, cov = lightmap_texels(QUAD_P, QUAD_N, QUAD_T, QUAD_I, 8, 8)
    assert pts.shape == nrm.shape == (8, 8, 3) and pts.dtype == nrm.dtype == np.float32 and cov.shape == (8, 8) and cov.dtype == bool
    assert cov.all()
    for y in range(8):
        for x in range(8):
            u, v = (x + 0.5) / 8, 1 - (y + 0.5) / 8
            assert np.allclose(pts[y, x], (2 * u - 1, 0, 1 - 2 * v), rtol=0, atol=1e-6), (x, y)
    assert np.array_equal(nrm, np.broadcast_to(np.float32([0, 1, 0]), nrm.shape))
    # flat and shaped inputs are the same mesh; an empty index list covers nothing
    again = lightmap_texels(QUAD_P.reshape(-1), QUAD_N.reshape(-1), QUAD_T.reshape(-1), QUAD_I.reshape(-1), 8, 8)
    assert all(np.array_equal(a, b) for a, b in zip(again, (pts, nrm, cov)))
    p0, n0, c0 = lightmap_texels(QUAD_P, QUAD_N, QUAD_T, np.zeros((0, 3), np.uint32), 5, 3)
    assert not c0.any() and not p0.any() and not n0.any() and p0.shape == (3, 5, 3)
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            lightmap_texels(QUAD_P, QUAD_N, QUAD_T, QUAD_I, *bad)


def test_lightmap_texels_shared_diagonal_goes_to_the_lower_triangle():
    """At 8 x 8 the centres of the texels x = 7 - y lie exactly on the quad's diagonal u = v (both edge functions are exactly zero there).
    The two triangles of a flat face interpolate the same point and normal on their common edge, so the winner cannot be seen on the
    cube; here the two triangles have vertices of their own with different normals, and swapping them swaps the diagonal's normal."""
    from cs397raytracingsp22_amd import lightmap_texels
    P = np.concatenate([QUAD_P[[0, 1, 2]], QUAD_P[[0, 2, 3]]])
    T = np.concatenate([QUAD_T[[0, 1, 2]], QUAD_T[[0, 2, 3]]])
    N = np.float32([[0, 1, 0]] * 3 + [[1, 0, 0]] * 3)
    for order, first in ((np.uint32([[0, 1, 2], [3, 4, 5]]), (0, 1, 0)), (np.uint32([[3, 4, 5], [0, 1, 2]]), (1, 0, 0))):
        _, nrm, cov = lightmap_texels(P, N, T, order, 8, 8)
        assert cov.all()
        for y in range(8):
            assert tuple(nrm[y, 7 - y]) == first, (y, first)
            if y < 7:                                                          # off the diagonal each triangle keeps its own texels
                assert tuple(nrm[y + 1, 7 - y]) == (0, 1, 0) and tuple(nrm[y, 6 - y]) == (1, 0, 0)


def _cube():
    from cs397raytracingsp22_amd import objload
    with gzip.open(os.path.join(ROOT, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
        return objload.load_obj_text(fh.read())[0]


def _containing(mesh, u, v):
    """Indices of the triangles whose uv triangle holds (u, v), edges included: the test's own statement of coverage."""
    T = mesh.texcoords.reshape(-1, 2).astype(np.float64)
    out = []
    for k, (a, b, c) in enumerate(mesh.indices.reshape(-1, 3)):
        def edge(p, q):
            return (T[q][0] - T[p][0]) * (v - T[p][1]) - (T[q][1] - T[p][1]) * (u - T[p][0])
        e = np.array([edge(a, b), edge(b, c), edge(c, a)])
        if (e >= 0).all() or (e <= 0).all():
            out.append(k)
    return out


@pytest.mark.parametrize("W,H", [(32, 32), (37, 19)])
def test_lightmap_texels_cube_inverts_the_oracles_texture_sampler(orc, W, H):
    from cs397raytracingsp22_amd import Texture, lightmap_texels
    mesh = _cube()
    P, N, T = mesh.positions.reshape(-1, 3), mesh.normals.reshape(-1, 3), mesh.texcoords.reshape(-1, 2)
    pts, nrm, cov = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H)
    # the cube's atlas: six squares of side 1/3 in a 3 x 2 grid, the strip v > 2/3 ... holds the rest; most of the map is covered
    assert 0.5 * W * H <= cov.sum() <= W * H
    xy = np.zeros((H, W, 3), np.uint8)
    xy[..., 0] = np.arange(W)[None, :]
    xy[..., 1] = np.arange(H)[:, None]
    tex = Texture(xy)                                                         # pixel (x, y) stores (x, y, 0)
    tri = mesh.indices.reshape(-1, 3)
    seen_tie = 0
    for y in range(H):
        for x in range(W):
            u, v = (x + 0.5) / W, 1 - (y + 0.5) / H
            inside = _containing(mesh, u, v)
            assert bool(cov[y, x]) == bool(inside), (x, y)
            if not inside:
                assert not nrm[y, x].any() and not pts[y, x].any() and not np.signbit(nrm[y, x]).any()      # zero normal, zero point
                continue
            # the point is the interpolation inside the LOWEST containing triangle (on the cube a tie is invisible unless the two
            # triangles belong to different faces); recover its barycentrics from the point and interpolate the uv with them
            a, b, c = tri[inside[0]]
            seen_tie += len(inside) > 1
            A = np.stack([P[a], P[b], P[c]], axis=1).astype(np.float64)
            w, *_ = np.linalg.lstsq(np.vstack([A, np.ones(3)]), np.append(pts[y, x].astype(np.float64), 1.0), rcond=None)
            assert w.min() >= -1e-5 and abs(w.sum() - 1) <= 1e-6, (x, y, w)
            uv = w @ T[[a, b, c]].astype(np.float64)
            got = orc.texture_sample(tex, float(uv[0]), float(uv[1]))
            assert (int(round(got[0] * 255)), int(round(got[1] * 255))) == (x, y), (x, y, uv)
            assert np.allclose(nrm[y, x], N[a], atol=1e-6) and abs(float(np.linalg.norm(nrm[y, x].astype(np.float64))) - 1) <= 1e-6
    print(f"cube {W}x{H}: {int(cov.sum())} of {W * H} texels covered, {seen_tie} texel centres on a shared edge")


def test_lightmap_texels_transform_and_offset():
    from cs397raytracingsp22_amd import cgmath, lightmap_texels
    mesh = _cube()
    W = H = 32
    base_p, base_n, cov = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H)
    M = cgmath.mul(cgmath.from_translation((0.5, -2.0, 3.0)), cgmath.from_angle_y(30.0), cgmath.from_angle_x(-20.0),
                   cgmath.from_nonuniform_scale(2.0, 0.5, 3.0))
    pts, nrm, cov2 = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H, transform=M)
    assert np.array_equal(cov, cov2)                                          # coverage is decided in uv space
    M64 = M.astype(np.float64)
    want = base_p.astype(np.float64) @ M64[:3, :3].T + M64[:3, 3]
    assert np.abs(pts[cov] - want[cov]).max() <= 1e-5
    length = np.linalg.norm(nrm[cov].astype(np.float64), axis=-1)
    assert np.abs(length - 1).max() <= 1e-6                                   # unit normals in spite of the non-uniform scale ...
    # ... and perpendicular to the transformed face: to the images of two edge directions of the face the texel lies on
    for y, x in zip(*np.nonzero(cov)):
        n0 = base_n[y, x].astype(np.float64)
        t1 = np.roll(n0, 1)                                                   # the cube's faces are axis-aligned: two tangents of the face
        t2 = np.roll(n0, 2)
        for t in (t1, t2):
            assert abs(float(nrm[y, x].astype(np.float64) @ (M64[:3, :3] @ t))) <= 1e-6, (x, y)
        assert float(nrm[y, x].astype(np.float64) @ (M64[:3, :3] @ n0)) > 0   # the outward side stays outward
    assert not pts[~cov].any() and not nrm[~cov].any()
    # offset: exactly that far along the normal (up to the f32 rounding of the result)
    for off in (1e-3, 0.25):
        moved, n2, _ = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H, transform=M, offset=off)
        assert np.array_equal(n2, nrm)
        step = moved[cov].astype(np.float64) - pts[cov].astype(np.float64)
        assert np.abs(step - off * nrm[cov].astype(np.float64)).max() <= 2e-6     # two f32 roundings of coordinates below 8 (ulp 2^-21) and the f64 slack
        assert not moved[~cov].any()                                          # an empty texel stays the zero point
