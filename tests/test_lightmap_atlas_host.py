"""Lightmap atlas (mi_lightmap_texels / mi_lightmap_texels_device / mi_bake_lightmap): what can be checked without a GPU — the jitter
stream's numpy restatement against the oracle's generator, the jittered form of the host helper lightmap_texels against a per-sample
brute force, the three prototypes in the header and its mirrors, and every refusal of the host form that comes before the context is
looked at (the library checks a call's arguments first, so a NULL context reports them as a device would)."""
import ctypes as C
import gzip
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["mi_lightmap_texels", "mi_lightmap_texels_device", "mi_bake_lightmap"]
U32, F32 = ("uint32_t", "u32"), ("float", "f32")
TEXELS = [("mi_ctx*", "*mut mi_ctx"), ("const mi_mesh*", "*const mi_mesh"), U32, U32, U32, U32, U32, F32,
          ("float*", "*mut f32"), ("float*", "*mut f32"), ("int32_t*", "*mut i32")]
PARAMS = {
    "mi_lightmap_texels": TEXELS,
    "mi_lightmap_texels_device": TEXELS + [("void*", "*mut c_void")],
    "mi_bake_lightmap": [("mi_ctx*", "*mut mi_ctx"), ("const mi_camera_desc*", "*const mi_camera_desc"),
                         ("const mi_render_opts*", "*const mi_render_opts"), ("const mi_mesh*", "*const mi_mesh"), U32, F32,
                         ("float*", "*mut f32"), ("uint8_t*", "*mut u8"), ("uint32_t*", "*mut u32"), ("int32_t*", "*mut i32"),
                         ("mi_stats*", "*mut mi_stats")],
}

QUAD_P = np.float32([[-1, 0, 1], [1, 0, 1], [1, 0, -1], [-1, 0, -1]])          # uv (0,0) (1,0) (1,1) (0,1)
QUAD_N = np.float32([[0, 1, 0]] * 4)
QUAD_T = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]])
QUAD_I = np.uint32([[0, 1, 2], [0, 2, 3]])


def _cube():
    from cs397raytracingsp22_amd import objload
    with gzip.open(os.path.join(ROOT, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
        return objload.load_obj_text(fh.read())[0]


# ---------------------------------------------------------------- the jitter stream
def test_lightmap_jitter_is_the_oracles_stream(orc):
    from cs397raytracingsp22_amd import lightmap_jitter
    W, H, R = 7, 5, 3
    for seed in (0, 9, 0xfffffffe):
        j = lightmap_jitter(W, H, R, seed)
        assert j.shape == (R, H, W, 2) and j.dtype == np.float32
        for r in range(R):
            for y in range(H):
                for x in range(W):
                    words = np.asarray(orc.rng_words(seed, 2 * W * H + y * W + x, r, 2), np.uint32)
                    want = ((words >> np.uint32(9)) | np.uint32(0x3f800000)).view(np.float32) * np.float32(1.0) + np.float32(0.0 - 1.0)
                    assert np.array_equal(j[r, y, x].view(np.uint32), want.view(np.uint32)), (seed, r, y, x)
        assert (j >= 0).all() and (j < 1).all()
    for bad in ((0, 5, 1), (7, 0, 1), (7, 5, 0)):
        with pytest.raises(ValueError):
            lightmap_jitter(*bad, 1)
    with pytest.raises(ValueError):
        lightmap_jitter(32768, 32768, 1, 1)                                    # 3 W H > 2^31, refused before anything is allocated


# ---------------------------------------------------------------- the helper's jittered form
def test_half_jitter_is_the_default_call_bit_for_bit():
    from cs397raytracingsp22_amd import lightmap_texels
    mesh = _cube()
    W, H = 33, 17
    base = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H, offset=1e-3)
    got = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H, offset=1e-3,
                          jitter=np.full((1, H, W, 2), 0.5, np.float32))
    assert base[2].any() and not base[2].all()
    for a, b in zip(base, got):
        assert b.shape == (1,) + a.shape and b.dtype == a.dtype
        assert np.array_equal(a.view(np.uint8), b[0].view(np.uint8))
    # with_triangle alone: the same three tables, and the winner's index where covered
    p, n, c, t = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, W, H, offset=1e-3, with_triangle=True)
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(base, (p, n, c)))
    assert t.dtype == np.int32 and np.array_equal(t >= 0, c) and (t[~c] == -1).all() and t.max() < mesh.n_triangles


def test_jittered_quad_against_a_per_sample_brute_force():
    from cs397raytracingsp22_amd import lightmap_jitter, lightmap_texels
    W = H = 8
    R = 5
    # the quad's corners pulled inside the atlas, so that jittered samples fall off it as well, and two further triangles on top
    T = np.float32(QUAD_T * 0.8 + 0.07)
    P = np.concatenate([QUAD_P, QUAD_P + np.float32([0, 1, 0])])
    N = np.concatenate([QUAD_N, np.float32([[1, 0, 0]] * 4)])
    T2 = np.concatenate([T, np.float32([[0.3, 0.2], [0.9, 0.4], [0.5, 0.95], [0.1, 0.6]])])
    I = np.uint32([[0, 1, 2], [4, 5, 6], [0, 2, 3], [6, 4, 7]])              # overlapping: the lowest index has to win
    J = lightmap_jitter(W, H, R, 5)
    pts, nrm, cov, tri = lightmap_texels(P, N, T2, I, W, H, jitter=J, with_triangle=True)
    assert pts.shape == (R, H, W, 3) and tri.shape == cov.shape == (R, H, W)
    P64, T64 = P.astype(np.float64), T2.astype(np.float64)
    winners = set()
    for r in range(R):
        for y in range(H):
            for x in range(W):
                u = (x + float(J[r, y, x, 0])) / W
                v = 1.0 - (y + float(J[r, y, x, 1])) / H
                want, wpt = -1, np.zeros(3)
                for k, (a, b, c) in enumerate(I):
                    (ua, va), (ub, vb), (uc, vc) = T64[a], T64[b], T64[c]
                    area = (ub - ua) * (vc - va) - (vb - va) * (uc - ua)
                    s = 1.0 if area > 0 else -1.0
                    ea = ((ub - u) * (vc - v) - (vb - v) * (uc - u)) * s
                    eb = ((uc - u) * (va - v) - (vc - v) * (ua - u)) * s
                    ec = ((ua - u) * (vb - v) - (va - v) * (ub - u)) * s
                    if ea >= 0 and eb >= 0 and ec >= 0:
                        tot = ea + eb + ec
                        want, wpt = k, ea / tot * P64[a] + eb / tot * P64[b] + ec / tot * P64[c]
                        break
                assert tri[r, y, x] == want and bool(cov[r, y, x]) == (want >= 0), (r, y, x)
                assert np.array_equal(pts[r, y, x], wpt.astype(np.float32)), (r, y, x)
                winners.add(want)
    assert winners == {-1, 0, 1, 2, 3}                                         # every triangle wins somewhere and some samples miss
    assert (tri != tri[0]).any()                                               # and the rows differ
    with pytest.raises(ValueError):
        lightmap_texels(P, N, T2, I, W, H, jitter=J[:, :, :7])


# ---------------------------------------------------------------- prototypes and mirrors
def _c_types(args):
    return [" ".join(re.match(r"(.+?)\s*\w+$", " ".join(a.split())).group(1).split()) for a in args.split(",")]


def test_header_and_mirrors_agree_on_the_three_prototypes():
    from cs397raytracingsp22_amd import abi
    hdr = open(os.path.join(ROOT, "include", "mi_rt.h")).read()
    assert re.search(r"#define\s+MI_RT_ABI_VERSION\s+5\b", hdr) and re.search(r"#define\s+MI_LM_JITTER\s+1u\b", hdr)
    assert abi.MI_LM_JITTER == 1
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "src", "util", "mi_rt.rs")).read()
    block = re.search(r'extern\s+"C"\s*\{(.*?)\n\}', rust, flags=re.S).group(1)
    lib = abi.load()
    raw = C.CDLL(abi.LIB_PATH)
    for name in NAMES:
        args = re.search(rf"\bint\s+{name}\s*\(([^)]*)\)\s*;", code).group(1)
        assert _c_types(args) == [p[0] for p in PARAMS[name]], name
        rargs = re.search(rf"pub\s+fn\s+{name}\s*\(([^)]*)\)\s*->\s*c_int;", block).group(1)
        assert [" ".join(a.split(":", 1)[1].split()) for a in rargs.split(",")] == [p[1] for p in PARAMS[name]], name
        assert name in abi.EXPORTS and getattr(lib, name).restype is C.c_int and len(getattr(lib, name).argtypes) == len(PARAMS[name])
        assert C.cast(getattr(raw, name), C.c_void_p).value
    assert lib.mi_lightmap_texels.argtypes[7] is C.c_float and lib.mi_bake_lightmap.argtypes[5] is C.c_float
    doc = " ".join(re.sub(r"\n \*", "\n", hdr[hdr.index("lightmap atlas"):hdr.index("int  mi_lightmap_texels(")]).split())
    for phrase in ("[rows][H][W][3]", "(seed, 2*W*H + y*W + x, r)", "LOWEST triangle index", "3*W*H > 2^31", "MI_ERR_OOM",
                   "never the buffers mi_reserve sized", "inverse transpose", "without fused multiply-adds", "n_triangles * tiles"):
        assert phrase in doc, phrase
    wrapper = open(os.path.join(ROOT, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert re.search(r"pub fn bake_lightmap\(&self, ", wrapper) and "mi_rt::mi_bake_lightmap(" in wrapper
    hpp = open(os.path.join(ROOT, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    call = re.search(r"mi_bake_lightmap\(([^;]*)\);", hpp).group(1)
    assert "RgbImage bake_lightmap(" in hpp and len(call.split(",")) == len(PARAMS["mi_bake_lightmap"])
    import cs397raytracingsp22_amd as pkg
    for cls, names in ((pkg.Context, ("lightmap_texels", "lightmap_texels_device", "bake_lightmap")), (pkg.Scene, ("bake_lightmap",))):
        for n in names:
            assert callable(getattr(cls, n)), (cls, n)
    assert callable(pkg.lightmap_jitter)


def test_cpp_mirror_compiles_against_the_header(tmp_path):
    import subprocess
    src = tmp_path / "bl.cpp"
    src.write_text('#include "tracing.hpp"\nusing namespace cs397;\n'
                   "RgbImage (Scene::*bake)(const mi_mesh&, uint32_t, uint32_t, uint32_t, bool, float, uint32_t, int, mi_stats*) const = "
                   "&Scene::bake_lightmap;\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "cs397raytracingsp22_amd", "host"), str(src)], check=True)


# ---------------------------------------------------------------- refusals of the host form, no device needed
def test_host_form_refuses_bad_arguments_before_it_looks_at_the_context():
    from cs397raytracingsp22_amd import abi
    from cs397raytracingsp22_amd.tracing import mesh_pod
    lib = abi.load()
    mesh = _cube()
    pod, keep = mesh_pod(mesh)
    out = np.full((2, 4, 4, 3), -7.0, np.float32)
    tri = np.full((4, 4), -7, np.int32)
    nan = float("nan")

    def call(mesh=pod, w=4, h=4, rows=1, flags=0, offset=0.0, pts=out[0].ctypes.data, nrm=out[1].ctypes.data, device=False):
        m = C.byref(mesh) if mesh is not None else None
        if device:
            rc = lib.mi_lightmap_texels_device(None, m, w, h, rows, flags, 1, offset, pts, nrm, tri.ctypes.data, None)
        else:
            rc = lib.mi_lightmap_texels(None, m, w, h, rows, flags, 1, offset, pts, nrm, tri.ctypes.data)
        msg = lib.mi_last_error().decode()
        assert rc == abi.MI_ERR_INVALID and len(msg) > 10, (rc, msg)
        return msg

    for device in (False, True):
        who = "mi_lightmap_texels_device" if device else "mi_lightmap_texels"
        assert call(device=device) == "ctx is NULL"                              # all arguments good: only the context is missing
        assert "mesh is NULL" in call(mesh=None, device=device)
        for w, h in ((0, 4), (4, 0), (32769, 4), (4, 32769)):
            assert "1 .. 32768" in call(w=w, h=h, device=device)
        for rows in (0, 65536):
            assert "1 .. 65535" in call(rows=rows, device=device)
        assert "unknown flag" in call(flags=2, device=device) and "unknown flag" in call(flags=abi.MI_LM_JITTER | 4, device=device)
        assert "NaN" in call(offset=nan, device=device)
        assert "out_points" in call(pts=None, device=device) and "out_points" in call(nrm=None, device=device)
        assert "exceeds 2^31" in call(w=32768, h=32768, device=device)
        assert call(w=32768, h=21845, device=device) == "ctx is NULL"             # 3 W H = 2^31 - 32768: allowed
        assert call(flags=abi.MI_LM_JITTER, rows=65535, offset=float("inf"), device=device) == "ctx is NULL"
        for field in ("positions", "normals", "texcoords", "indices"):
            bad, _ = mesh_pod(mesh)
            setattr(bad, field, type(getattr(bad, field))())
            assert "required" in call(mesh=bad, device=device), field
        bad, _ = mesh_pod(mesh)
        bad.n_triangles = -1
        assert who in call(mesh=bad, device=device)
    # a mesh of no triangles needs no index array
    empty, _ = mesh_pod(mesh)
    empty.n_triangles, empty.indices = 0, type(empty.indices)()
    assert call(mesh=empty) == "ctx is NULL"
    assert np.all(out == -7.0) and np.all(tri == -7)                               # nothing was written
    del keep


def test_python_mirror_refuses_a_malformed_mesh_before_any_library_call():
    from cs397raytracingsp22_amd import Context, objload
    ctx = Context.__new__(Context)                                                 # no mi_ctx_create: a library call would fail on the missing handle
    mesh = _cube()
    broken = objload.Mesh(mesh.positions, mesh.normals[:-3], mesh.texcoords, mesh.indices)
    with pytest.raises(ValueError):
        Context.lightmap_texels(ctx, broken, 4, 4)
    with pytest.raises(ValueError):
        Context.bake_lightmap(ctx, None, broken)


def test_abi_census_still_holds():
    """tests/test_abi.py, unchanged, is the census; this pins the count it sees for the three additions."""
    from cs397raytracingsp22_amd import abi
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi_rt.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(mi_[a-z_0-9]+)\s*\(", hdr)))
    assert declared == sorted(abi.EXPORTS) and set(NAMES) <= set(declared)
