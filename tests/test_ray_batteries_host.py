"""The ray batteries of tests/ray_batteries.py, checked without a GPU: (1) each battery really contains the edge rays it claims (census,
counted by an f32 restatement of the expression in question); (2) each battery notices a mutated oracle — the table below changes ONE
comparison or constant of oracle/*.c at a time, and the named battery must get at least one ray that differs from the true oracle;
(3) the oracle equals a float64 brute force without a tree on the robust rays of whole scenes (tests/f64_brute_force.py: the rule for
"robust", the measured robust shares and distance figures, and the bars are in its docstring).

Float64 brute force, measured (robust share camera / bounce; largest relative distance difference camera / bounce): config1 0.9820 / 0.9973,
2.2e-06 / 2.2e-02; config2 0.9860 / 0.9963, 3.1e-06 / 2.9e-03; config5 0.9873 / 0.9975, 5.4e-06 / 1.2e-03; head_scene 0.9887 / 0.9893,
6.2e-06 / 7.0e-03.  Bars: 4 x the largest = 2.5e-05 (camera) and 9.0e-02 (bounce); robust shares required: 0.97 and 0.90."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import ray_batteries as rb
from test_scene_compile_host import Blob, shim  # noqa: F401  (the scene compiler on the CPU and the decoder of its blob)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE = os.path.join(ROOT, "oracle")
SEED = 3


# ---------------------------------------------------------------- census
def positive(census, skip=()):
    for k, v in census.items():
        if k in skip or not isinstance(v, (int, np.integer)):
            continue
        assert v >= 1, (k, v)


def test_census_sphere():
    _, o, d, calls, c = rb.sphere_battery()
    print(c)
    positive(c)
    assert 200 <= len(o) <= 999 and len(o) % 64 == 5 and len(calls) >= 4


def test_census_triangle():
    sc, o, d, calls, c = rb.triangle_battery()
    print(c)
    positive(c)
    assert len(sc.objects) % 2 == 1            # pairs plus an odd tail
    assert 200 <= len(o) <= 999


def test_census_plane():
    _, o, d, calls, c = rb.plane_battery()
    print(c)
    positive(c)
    assert 200 <= len(o) <= 999


def test_census_window():
    _, o, d, calls, c = rb.window_battery(1.0)
    print(c)
    positive(c)
    assert len(o) == 64 and len(calls) == 10
    tmins, tmaxs = {a for a, _, _ in calls}, {b for _, b, _ in calls}
    one = np.float32(1.0)
    assert {1.0, float(np.nextafter(one, np.float32(2))), 0.0, -1.0} <= tmins
    assert {1.0, float(np.nextafter(one, np.float32(0))), rb.INF, rb.FMAX} <= tmaxs


def test_census_magnitude():
    _, o, d, calls, c = rb.magnitude_battery()
    ks = set(c["ks"])
    for centre in (-126, -125, 125, 126):
        for k in range(centre - 3, centre + 4):
            assert k in ks or k > 126, k
    assert min(ks) == -140 and max(ks) == 126
    print(c["classes seen"])
    assert set(c["classes seen"]["a"]) == {"zero", "denormal", "normal", "inf"}
    assert set(c["classes seen"]["bb"]) >= {"zero", "normal", "inf"}
    assert set(c["classes seen"]["fac"]) >= {"zero", "normal", "inf"}
    assert set(c["classes seen"]["g"]) >= {"denormal", "normal", "inf"}
    for k in c["ks"]:                          # each class set is recorded per k
        assert all(len(c["per_k"][k][n]) >= 1 for n in ("a", "bb", "fac", "g"))
    # every intermediate normal: a window of k around 0 and nothing near the range limits
    kn = set(c["k_of"][c["all_normal"]].tolist())
    assert 0 in kn and len(kn) >= 10 and all(abs(k) < 64 for k in kn), sorted(kn)
    assert 200 <= len(o) <= 999


def test_census_volume():
    _, o, d, calls, c = rb.volume_battery()
    print(c)
    positive(c)
    assert c["densities"] == [1e-3, 1.0, 1e3]
    assert 200 <= len(o) <= 999
    assert any(tm == 2.5 for _, tm, _ in calls)


@pytest.mark.parametrize("transform", sorted(rb.MESH_TRANSFORMS))
def test_census_mesh(transform):
    _, o, d, calls, c = rb.mesh_battery(transform)
    print(c)
    positive(c)
    assert 200 <= len(o) <= 999


def test_census_long_list(shim):
    """The waves' fate is counted with the top-level tree's own constants, read from the compiled scene (tests/test_scene_compile_host.py's
    decoder), through the restated two_stage_pad."""
    from test_gpu_ray_queries import long_triangle_list
    sc = rb.long_list_battery(long_triangle_list())[0]
    blob = Blob(shim, sc.flatten().desc)
    assert blob.top_meshf >= 0 and blob.n_list_lin < blob.n_list_tri           # the tree is there
    fc = blob.meshf[blob.top_meshf]
    fconst = {"E2": float(fc["E2"]), "L": float(fc["L"]), "c": [float(x) for x in fc["c"]], "R": float(fc["R"])}
    blob.close()
    sc, o, d, calls, c = rb.long_list_battery(long_triangle_list(), fconst)
    print(c)
    assert c["triangles"] >= 96 + 2 + 10
    assert c["waves of near rays only"] >= 3 and c["waves of far rays only"] >= 1 and c["waves mixing both kinds"] >= 1
    assert c["origin at 1e13"] >= 64 + 32
    assert c["ties: rays both duplicates accept at one distance"] >= 3
    assert [tm for _, tm, _ in calls] == [100.0, rb.INF, 1.0e14]
    n_waves = -(-len(o) // 64)
    for tm in (100.0, 1.0e14):                                                 # a finite t_max: every wave of near rays walks the tree
        assert c[f"t_max {tm}: waves covered entirely (tree walked)"] == c["waves of near rays only"] >= 4
        assert c[f"t_max {tm}: near rays refused"] == 0 and c[f"t_max {tm}: far rays covered"] == 0
        assert c[f"t_max {tm}: the ties' wave walks the tree"] == 1
        assert c[f"t_max {tm}: waves with a refused lane (plain loop)"] >= 2
    assert c[f"t_max {rb.INF}: waves covered entirely (tree walked)"] == 0       # +inf: refused, every wave takes the plain loop
    assert c[f"t_max {rb.INF}: waves with a refused lane (plain loop)"] == n_waves
    a, b = c["duplicate indices"]
    assert a < b and sc.objects[a].a == sc.objects[b].a


@pytest.mark.parametrize("size", rb.TEX_SIZES)
def test_census_texture(orc, size):
    W, H = size
    tex = rb.index_texture(W, H)
    assert tex.img.shape == (H, W, 3)
    x, y = W - 1, H - 1
    assert tuple(tex.img[y, x]) == (x & 255, y & 255, (x >> 8) | ((y >> 8) << 4))
    for uvs in rb.QUAD_UVS:
        _, o, d, calls, c = rb.texture_battery(size, uvs)
        print(c)
        assert c["rays"] >= 30 and c["hits"] >= 30
        positive(c, skip=("k/W targets",) + (rb.TEX_OUTSIDE_NOT_REQUIRED if uvs == "outside" else ()))
        want = {"unit": {"u == 0", "u == 0.999f", "u == 1"}, "outside": {"u == 0", "u == 1", "u < 0", "u > 1"}, "nan": {"u NaN", "v NaN"}}[uvs]
        if W > 1 and uvs != "nan":
            want |= {"u on k/W", "u on a texel boundary (clamp(u) * W an integer >= 1)"}
            if uvs == "unit":
                want |= {"u the f32 neighbour below k/W", "u the f32 neighbour above k/W", "u the last f32 before a texel boundary, in texel k - 1"}
        assert want <= set(c), want - set(c)
        # the census stands on quad_uv_terms: its uv is the oracle's, bit for bit
        sc = rb.texture_battery(size, uvs)[0]
        osc = orc.OracleScene(sc.flatten())
        hit, uv = rb.quad_uv_terms(o, d, sc.objects[0].mesh)
        for i in range(len(o)):
            r = osc.intersect(o[i], d[i], t_min=0.001, t_max=rb.INF, seed=SEED, pixel=i, sample=0)
            assert bool(r.hit) == bool(hit[i]), (uvs, i)
            if r.hit:
                assert np.float32(r.uv[0]).tobytes() == uv[i, 0].tobytes() or (np.isnan(r.uv[0]) and np.isnan(uv[i, 0])), (uvs, i, r.uv[0], uv[i, 0])
                assert np.float32(r.uv[1]).tobytes() == uv[i, 1].tobytes() or (np.isnan(r.uv[1]) and np.isnan(uv[i, 1])), (uvs, i, r.uv[1], uv[i, 1])
        osc.close()
    # the integer restatement: truncation, saturation, NaN -> 0
    tx, ty = rb.texel_of_uv([[0.0, 0.0], [1.0, 1.0], [float("nan"), float("nan")], [-3.0, 7.0], [0.999, 0.5]], W, H)
    assert tx[0] == 0 and ty[0] == H - 1 and tx[2] == 0 and ty[2] == 0 and tx[3] == 0
    assert tx[1] == min(int(np.float32(0.999) * np.float32(W)), W - 1)


@pytest.mark.parametrize("kind", ["spheres", "triangles", "planes", "mesh", "mixed"])
def test_census_nonfinite(kind):
    _, o, d, calls, c = rb.nonfinite_battery(kind)
    print(c)
    positive(c)


# ---------------------------------------------------------------- sensitivity: oracle mutants
def hits(osc, o, d, calls):
    out = []
    for t_min, t_max, key in calls:
        for i in range(len(o)):
            r = osc.intersect(o[i], d[i], t_min=t_min, t_max=t_max, seed=SEED, pixel=key + i, sample=0)
            out.append((r.object if r.hit else -1, np.float32(r.distance).tobytes() if r.hit else b"", bytes(r.material) if r.hit else b""))
    return out


def battery(name):
    if name == "sphere":
        return rb.sphere_battery()
    if name == "triangle":
        return rb.triangle_battery()
    if name == "plane":
        return rb.plane_battery()
    if name == "window":
        return rb.window_battery(1.0)
    if name == "magnitude":
        return rb.magnitude_battery()
    if name == "volume":
        return rb.volume_battery()
    if name == "mesh":
        return rb.mesh_battery("identity")
    if name == "texture":
        return rb.texture_battery((2048, 2), "outside")
    raise KeyError(name)


# (file, old text — exactly once in the file, new text, the battery that must notice)
G = "orc_geometry.c"
MUTANTS = [
    ("sphere disc < 0 -> <=", G, "if (d < 0.0f) return 0;", "if (d <= 0.0f) return 0;", "sphere"),
    ("sphere t1 >= t_min -> >", G, "(t1 >= t_min)", "(t1 > t_min)", "sphere"),
    ("sphere t > t_max -> >=", G, "t > t_max) return 0;                             /* :410 */", "t >= t_max) return 0;   /* :410 */", "sphere"),
    ("sphere t < t_min -> <=", G, "if (t < t_min || t > t_max) return 0;                             /* :410 */", "if (t <= t_min || t > t_max) return 0;", "window"),
    ("Triangle u < 0 -> <=", G, "if (u < 0.0f) return 0;                                           /* :442 */", "if (u <= 0.0f) return 0;", "triangle"),
    ("Triangle v < 0 -> <=", G, "if (v < 0.0f || u + v > 1.0f) return 0;                           /* :445 */", "if (v <= 0.0f || u + v > 1.0f) return 0;", "triangle"),
    ("Triangle u + v > 1 -> >=", G, "u + v > 1.0f) return 0;                           /* :445 */", "u + v >= 1.0f) return 0;", "triangle"),
    ("Triangle |a| < EPSILON -> <=", G, "if (fabsf(a) < EPSILON) return 0;", "if (fabsf(a) <= EPSILON) return 0;", "triangle"),
    ("Triangle t > t_max -> >=", G, "t > t_max) return 0;                             /* :447 */", "t >= t_max) return 0;", "triangle"),
    ("Triangle t < t_min -> <=", G, "if (t < t_min || t > t_max) return 0;                             /* :447 */", "if (t <= t_min || t > t_max) return 0;", "triangle"),
    ("mesh u < 0 -> <=", G, "if (u < 0.0f) return 0;                                           /* :344 */", "if (u <= 0.0f) return 0;", "mesh"),
    ("mesh v < 0 -> <=", G, "if (v < 0.0f || u + v > 1.0f) return 0;                           /* :347 */", "if (v <= 0.0f || u + v > 1.0f) return 0;", "mesh"),
    ("mesh u + v > 1 -> >=", G, "u + v > 1.0f) return 0;                           /* :347 */", "u + v >= 1.0f) return 0;", "mesh"),
    ("mesh |g| < EPSILON -> <=", G, "if (fabsf(g) < EPSILON) return 0;", "if (fabsf(g) <= EPSILON) return 0;", "mesh"),
    ("mesh t > t_max -> >=", G, "t > t_max) return 0;                             /* :349 */", "t >= t_max) return 0;", "window"),
    ("mesh t < t_min -> <=", G, "if (t < t_min || t > t_max) return 0;                             /* :349 */", "if (t <= t_min || t > t_max) return 0;", "window"),
    ("plane d >= 0 -> >", G, "if (d >= 0.0f) return 0;", "if (d > 0.0f) return 0;", "plane"),
    ("plane t > t_max -> >=", G, "t > t_max) return 0;                             /* :485 */", "t >= t_max) return 0;", "plane"),
    ("plane t < t_min -> <=", G, "if (t < t_min || t > t_max) return 0;                             /* :485 */", "if (t <= t_min || t > t_max) return 0;", "plane"),
    ("AABB tmax <= tmin -> <", G, "if (tmax <= tmin) return 0;", "if (tmax < tmin) return 0;", "mesh"),
    ("volume restart 0.0001 -> 0.001", G, "t_entr + 0.0001f", "t_entr + 0.001f", "volume"),
    ("volume t_exit < t_min -> <=", G, "if (t_exit < t_min || t_entr > t_max) return 0;", "if (t_exit <= t_min || t_entr > t_max) return 0;", "volume"),
    ("volume t_entr > t_max -> >=", G, "t_entr > t_max) return 0;", "t_entr >= t_max) return 0;", "volume"),
    ("Scene closest hit < -> <=", "orc_tracing.c", "else if (hit.distance < best_hit.distance) best_hit = hit;   /* :335-336 */\n        }\n    }\n    if (have_best) *out = best_hit;\n    return have_best;                                                 /* :345 */",
     "else if (hit.distance <= best_hit.distance) best_hit = hit;\n        }\n    }\n    if (have_best) *out = best_hit;\n    return have_best;", "triangle"),
    ("texture clamp 0.999 -> 1.0", "orc_texture.c", "uv.x, 0.0f, 0.999f", "uv.x, 0.0f, 1.0f", "texture"),
    ("d normalised before the list test", "orc_tracing.c", "ray.direction = v3_from(dir);\n    orc_rayhit h;", "ray.direction = v3_normalize(v3_from(dir));\n    orc_rayhit h;", "magnitude"),
]
# The two window tests of the volume (geometry.rs:512) reject BEFORE the volume's random draw: on their own object `>=` / `<=` change nothing
# (dist_in_volume <= 0 either way), but they skip a draw, and every volume listed later then scatters elsewhere.  The volume battery holds
# rays with the earlier-listed volume exactly on the window's edge and a later-listed one inside it.


@pytest.fixture(scope="module")
def true_answers(orc):
    cache = {}

    def get(name):
        if name not in cache:
            sc, o, d, calls, _ = battery(name)
            osc = orc.OracleScene(sc.flatten())
            cache[name] = hits(osc, o, d, calls)
            osc.close()
        return cache[name]
    return get


def makefile_var(name):
    """A variable of oracle/Makefile (`NAME ?= words` or `NAME := words`)."""
    for line in open(os.path.join(ORACLE, "Makefile")).read().splitlines():
        head, sep, tail = line.partition("=")
        if sep and head.rstrip("?: \t") == name:
            return tail.split()
    raise KeyError(name)


@pytest.fixture(scope="module")
def oracle_objects(tmp_path_factory):
    """oracle/*.c and *.h copied once, every source compiled once to an object with the compiler, flags and source list of oracle/Makefile:
    a mutant recompiles only the file it changes and links it with the others' objects."""
    top = tmp_path_factory.mktemp("mutants")
    src = top / "oracle"
    src.mkdir()
    for f in os.listdir(ORACLE):
        if f.endswith((".c", ".h")):
            shutil.copy(os.path.join(ORACLE, f), src / f)
    (top / "include").mkdir()
    shutil.copy(os.path.join(ROOT, "include", "mi_rt.h"), top / "include" / "mi_rt.h")
    cc, flags, srcs = makefile_var("CC"), makefile_var("CFLAGS"), makefile_var("SRCS")
    for f in srcs:
        subprocess.run(cc + flags + ["-c", f, "-o", f + ".o"], cwd=src, check=True)
    return src, cc, flags, srcs


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_battery_notices_the_mutant(orc, true_answers, oracle_objects, mutant):
    title, fname, old, new, name = mutant
    src, cc, flags, srcs = oracle_objects
    text = (src / fname).read_text()
    assert text.count(old) == 1, (title, text.count(old))
    k = MUTANTS.index(mutant)
    changed = "mutant_%d_%s" % (k, fname)
    (src / changed).write_text(text.replace(old, new))
    so = src / ("liborc_mutant_%d.so" % k)
    subprocess.run(cc + flags + ["-c", changed, "-o", changed + ".o"], cwd=src, check=True)
    subprocess.run(cc + flags + ["-shared", "-o", str(so), changed + ".o"] + [f + ".o" for f in srcs if f != fname] + ["-lm", "-lpthread"],
                   cwd=src, check=True)
    lib = orc.load(str(so))
    sc, o, d, calls, _ = battery(name)
    osc = orc.OracleScene(sc.flatten(), lib=lib)
    got = hits(osc, o, d, calls)
    osc.close()
    ref = true_answers(name)
    differ = sum(1 for a, b in zip(got, ref) if a != b)
    print(f"{title}: {differ} of {len(ref)} answers of the {name} battery differ")
    assert differ >= 1


# ---------------------------------------------------------------- float64 brute force on whole scenes
import f64_brute_force as bf  # noqa: E402


@pytest.mark.parametrize("name", sorted(bf.SCENES))
def test_oracle_equals_f64_brute_force_on_robust_rays(orc, name):
    m = bf.measure(orc, name)
    for what, bar, share in (("camera", bf.BAR_CAMERA, 0.97), ("bounce", bf.BAR_BOUNCE, 0.90)):
        r = m[what]
        print(f"{name} {what}: {r['n']} rays, robust {r['robust']:.4f}, object mismatches on robust rays {r['mismatch']} (on all rays "
              f"{r['mismatch_all']}), distance: max rel {r['rel_max']:.3e}, p99 {r['rel_p99']:.3e}")
    for what, bar, share in (("camera", bf.BAR_CAMERA, 0.97), ("bounce", bf.BAR_BOUNCE, 0.90)):
        r = m[what]
        assert r["mismatch"] == 0, (what, r["bad"], r["obj"][r["bad"]], r["ref"][r["bad"]], r["dist"][r["bad"]], r["ref_dist"][r["bad"]])
        assert r["robust"] >= share, (what, r["robust"])
        assert r["rel_max"] <= bar, (what, r["rel_max"])
