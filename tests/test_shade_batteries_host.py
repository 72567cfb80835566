"""The shading batteries of tests/shade_batteries.py, checked without a GPU: (1) each battery really contains the edge rays and keys it
claims (census); the numpy restatement of the RNG stream equals the oracle's; (2) each battery notices a mutated oracle — the table below
changes ONE token of oracle/orc_materials.c, orc_tracing.c or orc_math.h at a time and the named batteries must get at least one orc_shade
answer that differs; (3) the oracle's estimator equals emission + dot_term * brdf * E(wall) / pdf computed in float64 from orc.scatter and
a float64 brute-force closest hit (tests/f64_brute_force.py) on the rays that are clear of every decision edge; (4) the GPU-free input
checker refuses what mi_shade_rays refuses.

One mutant of the issue's list is EQUIVALENT and therefore absent: removing the `fminf(.., 1.0f)` of materials.rs:81 changes no decision,
because for cosv > 1 the clamped product is eta * sqrtf(0) = 0 (or NaN for an infinite eta) and the unclamped one is eta * sqrtf(negative)
= NaN: `> 1.0f` is false for both.  The `fminf(.., 1.0f)` of refract (tracing.rs:65) is observable and is mutated instead.

Float64 check, measured (rays kept / on-purpose rays / left out by the margin or robustness filter, largest relative deviation of orc_shade
from the float64 value): see F64_MEASURED below; the bar is four times the largest."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import shade_batteries as sb
import f64_brute_force as bf
from test_ray_batteries_host import makefile_var, oracle_objects, positive  # noqa: F401  (the mutant machinery: sources compiled once per module)
from cs397raytracingsp22_amd import Camera, Dielectric, abi
from test_scene_compile_host import Blob, check_rotations, shim  # noqa: F401  (the scene compiler on the CPU and the decoder of its blob)

SEED = sb.SEED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family: (largest relative deviation measured, rays kept, share left out)
F64_MEASURED = {"lobe": 1.97e-07, "critical": 2.08e-07, "dot_term": 1.83e-07}
F64_BAR = 4 * max(F64_MEASURED.values())
F64_MAX_LEFT_OUT = 0.10


def shades(osc, bat):
    """orc_shade for every call and ray of a battery -> f32[calls, n, 3]."""
    sc, cam, o, d, calls, _ = bat
    out = []
    for key, depth, samples, tmax in calls:
        cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
        out.append(np.stack([osc.shade(cam, o[i], d[i], seed=SEED, pixel=key + i, sample=0) for i in range(len(o))]))
    return np.stack(out)


def differ(a, b):
    """Components that are not equal as f32 values (NaN equals NaN)."""
    return ~((a == b) | (np.isnan(a) & np.isnan(b)))


def show(label, census):
    print(label, {k: v for k, v in census.items() if not isinstance(v, np.ndarray)})


# ---------------------------------------------------------------- census
def test_rng_restatement_equals_the_oracle(orc):
    for key in (0, 1, 12345, 2 ** 26 - 1, 2 ** 32 - 1):
        assert np.array_equal(sb.rng_words(SEED, key, 16), orc.rng_words(SEED, key, 0, 16)), key
    assert np.array_equal(sb.rng_words(9, 77, 4), orc.rng_words(9, 77, 0, 4))
    keys = sb.keys_around(sb.U_TARGETS)
    print({u: v for u, v in keys.items()})
    for u, ks in keys.items():
        for k in ks:                                             # the found key's first gen01 IS the target, by the oracle's own words
            bits = int(orc.rng_words(SEED, k, 0, 1)[0])
            assert np.float32(np.uint32(0x3f800000 | bits >> 9).view(np.float32) - np.float32(1.0)) == np.float32(u), (u, k)
    assert len(keys[0.25]) >= 6 and len(keys[0.5]) >= 6 and len(keys[0.0]) >= 4
    for u in (0.25 - 2.0 ** -23, 0.25 + 2.0 ** -23, 0.5 - 2.0 ** -23, 0.5 + 2.0 ** -23, 2.0 ** -23):
        assert len(keys[u]) >= 2, u


def test_census_critical():
    eq = clamp = 0
    for label, bat in sb.all_batteries("critical"):
        c = bat[5]
        show(label, c)
        assert c["product < 1"] >= 1 and c["cosv > 1 (the clamp is active)"] >= 2 and c["cosv == 1"] >= 1, label
        assert c["product > 1"] >= 40 or (c["kind"] != "triangle" and c["ior"] > 1), label      # eta > 1 on some side of the probe
        assert 200 <= c["rays"] <= 999 and c["rays"] % 64 == 5
        if c["exact"]:
            eq += c["product == 1"]
        clamp += c["cosv > 1 (the clamp is active)"]
    print("critical: rays with eta * sqrt(1 - cosv^2) == 1 exactly:", eq)
    assert eq >= 5
    assert {1.25, 1.5, 2.0, 4.0, 8.0} <= set(sb.CRITICAL_IORS)
    front = sb.critical_battery(0.5, "plane")[5]
    assert front["backface (eta = ior)"] == 0 and front["product > 1"] >= 40           # the frontface counterpart: eta = 1 / ior = 2
    back = sb.critical_battery(2.0, "triangle")[5]
    assert back["backface (eta = ior)"] >= 80 and back["frontface (eta = 1 / ior)"] >= 40


def test_census_fresnel_draw():
    for label, bat in sb.all_batteries("fresnel"):
        c = bat[5]
        show(label, c)
        assert c["grazing rays with fresnel_factor == 1"] >= 1 and c["(ray, call): u == 0"] >= 2, label
        if c["ior"] == 3.0:
            assert c["fresnel_factor of the normal ray"] == 0.25
            for k in ("u < fresnel_factor", "u == fresnel_factor", "u > fresnel_factor", "u one step below fresnel_factor", "u one step above fresnel_factor"):
                assert c["(ray, call): " + k] >= 2, (label, k)
        elif c["ior"] == 1.0:
            assert c["fresnel_factor of the normal ray"] == 0.0 and c["(ray, call): u == fresnel_factor"] >= 2
        else:
            assert c["fresnel_factor of the normal ray"] == 1.0 and c["(ray, call): u > fresnel_factor"] == 0 and c["(ray, call): u == fresnel_factor"] == 0


def test_census_lobe():
    seen = set()
    for label, bat in list(sb.all_batteries("lobe")) + list(sb.all_batteries("lobe_kinds")):
        c = bat[5]
        show(label, c)
        seen.add((c["roughness"], c["metallic"]))
        if c["roughness"] == 1.0 and c["metallic"] in (0.75, 0.5) and c["exact"]:
            assert c["k_d of the normal ray"] == 1.0 - c["metallic"]
            for k in ("u < k_d", "u == k_d", "u > k_d", "u one step below k_d", "u one step above k_d", "diffuse lobe", "specular lobe"):
                assert c["(ray, call): " + k] >= 2, (label, k)
        if c["metallic"] == 1.0:
            assert c["(ray, call): diffuse lobe"] == 0 and c["(ray, call): u == 0"] >= 2 and c["(ray, call): u == k_d"] >= 2
        if c["metallic"] == 0.0 and c["roughness"] == 1.0:
            assert c["(ray, call): specular lobe"] == 0
        assert c["(ray, call): diffuse lobe"] + c["(ray, call): specular lobe"] >= 200
    assert {(0.0, 0.5), (0.5, 0.5), (2.0, 0.5), (1.0, -0.5), (1.0, 1.5), (1.0, 1.0), (1.0, 0.0)} <= seen


@pytest.mark.parametrize("form", ["plane", "triangle"])
def test_census_rotation(form):
    total = {"identity": 0, "pi": 0, "general": 0}
    edge = {"identity": set(), "pi": set(), "general": set()}
    for label, bat in sb.all_batteries("rotation_" + form):
        c = bat[5]
        show(label, c)
        for b in total:
            total[b] += c[b]
        for test, taken in (("n.y ulps from 1 (identity test)", "identity"), ("n.y / |n| ulps from -1 (pi test)", "pi")):
            if c[test] is not None and c[test] <= 8:
                edge[taken if c[taken] else "general"].add((taken, c[test]))
    print(form, "rays per branch of between_vectors:", total, "(test, ulps from its target) seen per branch taken:", {k: sorted(v) for k, v in edge.items()})
    assert all(v >= 8 for v in total.values()), total
    # both sides of ulps_eq's max_ulps = 4, for both of its uses
    assert ("identity", 4) in edge["identity"] and ("pi", 4) in edge["pi"]
    assert ("identity", 5) in edge["general"] and ("pi", 5) in edge["general"]
    for test in ("identity", "pi"):                                                # every count from 0 to 8, on the side ulps_eq puts it
        assert {(test, u) for u in range(5)} <= edge[test] and {(test, u) for u in range(5, 9)} <= edge["general"], (test, edge)
    if form == "plane":
        miss = [bat[5] for _, bat in sb.all_batteries("rotation_plane") if bat[5]["normal"] == (0.0, 0.0, 0.0)]
        assert len(miss) == 1 and miss[0]["probe hits"] == 0                                             # the zero normal is never hit
        lens = {bat[5]["normal"][1] for _, bat in sb.all_batteries("rotation_plane")}
        assert {0.5, 2.0, 2.0 ** -60} <= lens


def test_census_dot_term(orc):
    seen = {}
    for label, bat in sb.all_batteries("dot_term"):
        c = bat[5]
        show(label, c)
        seen[label] = c
    m0, m1, m2 = seen["dot_term metal0"], seen["dot_term metal1"], seen["dot_term metal2"]
    assert m0["clamp active (|new_d . n| > 1)"] >= 6 and m0["|new_d . n| <= 1"] >= 6 and m0["|d . n| below 2^-20 (parallel up to an ulp)"] >= 3
    assert m0["new_d . n < 0 (enters the object)"] == 0 and m1["new_d . n < 0 (enters the object)"] >= 8 and m2["new_d . n < 0 (enters the object)"] >= 8
    assert seen["dot_term tiny_normal"]["mag2(n) == 0 on a hit (the else arm)"] >= 100
    assert seen["dot_term zero_normal"]["probe hits"] == 0
    assert seen["dot_term volume"]["rays into the dense volume (hit normal zero: the else arm)"] >= 100
    # the volume's hit normal IS zero, by the oracle
    sc, cam, o, d, calls, _ = sb.dot_term_battery("volume")
    osc = orc.OracleScene(sc.flatten())
    zero = sum(1 for i in range(len(o)) if (lambda r: r.hit and r.object == sc.probe_index and not any(r.normal[:]))(osc.intersect(o[i], d[i], t_max=sb.INF, seed=SEED, pixel=i)))
    osc.close()
    print("dot_term volume: hits with a zero normal", zero)
    assert zero >= 100


def test_census_depth_and_nonfinite():
    c = sb.depth_battery()[5]
    show("depth", c)
    positive(c)
    assert c["segments of one axis ray, per call"][:5] == [0, 1, 2, 63, 64]
    depths = {(dp, s) for _, dp, s, _ in sb.DEPTH_CALLS}
    assert {(0, 1), (1, 1), (2, 1), (63, 1), (64, 1), (6, 2), (6, 3), (2, 64)} <= depths
    assert all(s == 1 for dp, s in depths if dp > 6)
    odd = 0
    for label, bat in sb.all_batteries("nonfinite"):
        c = bat[5]
        show(label, c)
        assert c["non-finite or denormal parameters of the probe or the walls"] + c["finite parameters outside the sane range (a negative ior)"] >= 1, label
        odd += c["finite parameters outside the sane range (a negative ior)"]
    assert odd == 1


def test_depth_battery_axis_rays_equal_the_mirror_series(orc):
    """The census's oracle-free hit counts, tied to orc_shade: an axis ray from the centre of the mirror room meets the centre of a face
    (on the shared diagonal of its two Triangles: the lower index wins), is sent straight back to the opposite face, and so on.  With
    h hits, Metal albedo a = 1 - 2^-6, pdf 1 and dot_term 1 the radiance is E_0 + a (E_1 + a (E_0 + ...)), h terms, whatever path_samples
    is (every sample repeats the path).  Computed in float64; orc_shade does at most 3 roundings per level (product, sum, the division by
    path_samples), so the bar is 3 h 2^-24 relative, per component."""
    sc, cam, o, d, calls, c = sb.depth_battery()
    osc = orc.OracleScene(sc.flatten())
    face_of = {(0, 0, -1): 0, (0, 0, 1): 1, (0, -1, 0): 2, (0, 1, 0): 3, (1, 0, 0): 4, (-1, 0, 0): 5}      # cube_mesh's quads
    a = 1.0 - 2.0 ** -6
    checked, worst = 0, 0.0
    for (key, depth, samples, tmax), h in zip(calls, c["hits along one axis path, per call"]):
        cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
        for i in np.flatnonzero(np.all(o == 0, axis=1))[:6]:
            ax = tuple(int(x) for x in d[i])
            E = [np.float64(sc.objects[2 * face_of[t]].material.emission) for t in (ax, tuple(-x for x in ax))]
            want = np.zeros(3)
            for lvl in reversed(range(h)):
                want = E[lvl % 2] + a * want
            got = np.float64(osc.shade(cam, o[i], d[i], seed=SEED, pixel=key + i, sample=0))
            if h == 0:
                assert not got.any(), (key, depth, tmax, i)
            else:
                dev = float(np.max(np.abs(got - want) / want))
                worst = max(worst, dev / (3 * h * 2.0 ** -24))
                assert dev <= 3 * h * 2.0 ** -24, (key, depth, samples, tmax, i, got, want)
            checked += 1
    osc.close()
    print(f"depth: {checked} axis (call, ray) pairs equal the mirror series; largest deviation {worst:.3f} of its bar")
    assert checked == 6 * len(calls)


def test_probe_kinds_are_hit_and_the_restated_normal_is_the_oracles(orc):
    """All four resolve_hit arms feed scatter: the probe of every kind is object scene.probe_index and the battery's rays hit it; for the exact kinds the
    census's facing normal and frontface are the oracle's, bit for bit."""
    for kind in sb.KINDS:
        sc, cam, o, d, calls, c = sb.lobe_battery(1.0, 0.5, kind)
        osc = orc.OracleScene(sc.flatten())
        nf, ff, hit = sb.facing(kind, o, d)
        hits = 0
        for i in range(len(o)):
            r = osc.intersect(o[i], d[i], t_max=sb.INF, seed=SEED, pixel=i)
            if r.hit and r.object == sc.probe_index:
                hits += 1
                if c["exact"]:
                    assert hit[i] and bool(r.frontface) == bool(ff[i]), (kind, i)
                    assert np.array_equal(np.float32(r.normal[:]), nf[i]), (kind, i, r.normal[:], nf[i])
            else:
                assert not hit[i] or not c["exact"], (kind, i)
        osc.close()
        print(kind, "probe hits", hits, "of", len(o))
        assert hits >= 150


def test_rotation_table_of_the_battery_scenes_equals_the_oracle(orc, shim):
    """The rotation the kernel READS for a list Triangle or a Plane (DScene.obj_rot, computed by the scene compiler on the host) for the
    edge normals of the rotation batteries: equal to the oracle's between_vectors bit for bit (zero signs and the identity flag as
    tests/test_scene_compile_host.py states them), and the compiled Triangle normal is the census's restated one."""
    entries = exempt = 0
    for fam in ("rotation_plane", "rotation_triangle"):
        for label, bat in sb.all_batteries(fam):
            flat = bat[0].flatten()
            b = Blob(shim, flat.desc)
            e, x = check_rotations(orc, flat.desc, b)
            entries, exempt = entries + e, exempt + x
            if fam == "rotation_triangle":
                assert np.array_equal(b.objs[0]["f"][9:12], np.float32(bat[5]["normal"])), (label, b.objs[0]["f"][9:12], bat[5]["normal"])
            b.close()
    print(f"rotation batteries: {entries} table entries equal the oracle's, {exempt} with the zero-sign exemption")
    assert entries == 2 * 13 * (sb.rotation_count("plane") + sb.rotation_count("triangle"))      # 13 list entries per scene, two sides each


# ---------------------------------------------------------------- sensitivity: oracle mutants
M, T, H = "orc_materials.c", "orc_tracing.c", "orc_math.h"
MUTANTS = [
    ("critical > 1 -> >= 1", M, "orc_powi2(cosv)) > 1.0f;", "orc_powi2(cosv)) >= 1.0f;", "critical"),
    ("refract: fminf(.., 1) removed", T, "float cos_theta = fminf(v3_dot(v3_neg(v), n), 1.0f);", "float cos_theta = v3_dot(v3_neg(v), n);", "critical"),
    ("eta: frontface arms swapped", M, "hit->frontface ? 1.0f / ior : ior", "hit->frontface ? ior : 1.0f / ior", "critical"),
    ("u >= fresnel_factor -> >", M, "orc_gen_range_01(&p->rng) >= fresnel_factor", "orc_gen_range_01(&p->rng) > fresnel_factor", "fresnel"),
    ("!critical_angle evaluated after the draw", M, "int will_refract = !critical_angle && (orc_gen_range_01(&p->rng) >= fresnel_factor);",
     "int will_refract = (orc_gen_range_01(&p->rng) >= fresnel_factor) && !critical_angle;", "critical"),
    ("u < k_d -> <=", M, "orc_gen_range_01(&p->rng) < k_d", "orc_gen_range_01(&p->rng) <= k_d", "lobe"),
    ("1 - roughness -> roughness", M, "fresnel * (1.0f - m->roughness)", "fresnel * (m->roughness)", "lobe"),
    ("fabsf(dir.y) -> dir.y", M, "dir.y = fabsf(dir.y);", "dir.y = dir.y;", "lobe"),
    ("ulps_eq max_ulps 4 -> 3 (identity test, plane form)", H, "return d <= 4;", "return d <= 3;", "rotation:identity:plane"),
    ("ulps_eq max_ulps 4 -> 3 (identity test, triangle form)", H, "return d <= 4;", "return d <= 3;", "rotation:identity:triangle"),
    ("ulps_eq max_ulps 4 -> 3 (pi test, plane form)", H, "return d <= 4;", "return d <= 3;", "rotation:pi:plane"),
    ("ulps_eq max_ulps 4 -> 3 (pi test, triangle form)", H, "return d <= 4;", "return d <= 3;", "rotation:pi:triangle"),
    ("mag2(n) > 0 -> >= 0", T, "(v3_mag2(hit.normal) > 0.0f)", "(v3_mag2(hit.normal) >= 0.0f)", "dot_term"),
    ("dot_term clamp: upper bound removed", T, "fabsf(v3_dot(new_ray.direction, hit.normal)), 0.0f, 1.0f)", "fabsf(v3_dot(new_ray.direction, hit.normal)), 0.0f, INFINITY)", "dot_term"),
    ("recursion_depth >= path_depth -> >", T, "if (recursion_depth >= cam->path_depth)", "if (recursion_depth > cam->path_depth)", "depth"),
    ("Dielectric emission returned", M, "if (m->kind == MI_MAT_DIELECTRIC) return v3_zero();", "if (0) return v3_zero();", "fresnel"),
    ("/ pdf -> * pdf", T, "v3_divs(v3_scale(v3_mul_elem(brdf_term, incoming_light), dot_term), pdf)", "v3_scale(v3_scale(v3_mul_elem(brdf_term, incoming_light), dot_term), pdf)", "lobe"),
    ("shade_ray t_min 0.001 -> 0", T, "orc_scene_intersect_ray(s, ray, 0.001f, cam->max_trace_dist", "orc_scene_intersect_ray(s, ray, 0.0f, cam->max_trace_dist", "depth"),
    ("integral / path_samples left out", T, "integral = v3_divs(integral, (float)cam->path_samples);", "integral = integral;", "depth"),
    ("ulps_eq max_ulps 4 -> 5 (identity test, plane form)", H, "return d <= 4;", "return d <= 5;", "rotation5:identity:plane"),
    ("ulps_eq max_ulps 4 -> 5 (identity test, triangle form)", H, "return d <= 4;", "return d <= 5;", "rotation5:identity:triangle"),
    ("ulps_eq max_ulps 4 -> 5 (pi test, plane form)", H, "return d <= 4;", "return d <= 5;", "rotation5:pi:plane"),
    ("ulps_eq max_ulps 4 -> 5 (pi test, triangle form)", H, "return d <= 4;", "return d <= 5;", "rotation5:pi:triangle"),
    ("max_trace_dist: t > t_max -> >= (list Triangle)", "orc_geometry.c", "t > t_max) return 0;                             /* :447 */", "t >= t_max) return 0;", "depth"),
]


def mutant_batteries(name):
    """(label, battery, mask or None) of the batteries that must notice a mutant; mask selects rays (by the census) whose answers count."""
    name, _, which = name.partition(":")
    which, _, form = which.partition(":")
    if name == "critical":
        return [(l, b, None) for l, b in sb.all_batteries("critical") if b[5]["kind"] in ("triangle", "plane")]
    if name == "fresnel":
        return [(l, b, None) for l, b in sb.all_batteries("fresnel") if b[5]["kind"] == "plane"]
    if name == "lobe":
        return [(f"lobe {r} {m}", sb.lobe_battery(r, m), None) for r, m in ((1.0, 0.75), (1.0, 0.5), (0.0, 0.5))]
    if name == "rotation":
        out = []
        for fam in ("rotation_" + form,):
            for l, b in sb.all_batteries(fam):
                test = {"identity": "n.y ulps from 1 (identity test)", "pi": "n.y / |n| ulps from -1 (pi test)"}[which]
                if b[5][test] in (3, 4, 5):
                    out.append((l, b, b[5]["branch"] == which))
        return out
    if name == "rotation5":                                        # the rays one ulp beyond the threshold: general now, taken by a max_ulps of 5
        out = []
        for fam in ("rotation_" + form,):
            for l, b in sb.all_batteries(fam):
                test, side = {"identity": ("n.y ulps from 1 (identity test)", "up"), "pi": ("n.y / |n| ulps from -1 (pi test)", "down")}[which]
                if b[5][test] == 5:
                    out.append((l, b, (b[5]["branch"] == "general") & b[5][side]))
        return out
    if name == "dot_term":
        return [(f"dot_term {v}", sb.dot_term_battery(v), None) for v in sb.DOT_VARIANTS]
    if name == "depth":
        return [("depth", sb.depth_battery(), None)]
    raise KeyError(name)


@pytest.fixture(scope="module")
def true_shades(orc):
    cache = {}

    def get(name):
        if name not in cache:
            res = []
            for label, bat, mask in mutant_batteries(name):
                osc = orc.OracleScene(bat[0].flatten())
                res.append(shades(osc, bat))
                osc.close()
            cache[name] = res
        return cache[name]
    return get


def build_mutant(oracle_objects, k, fname, old, new):
    src, cc, flags, srcs = oracle_objects
    text = (src / fname).read_text()
    assert text.count(old) == 1, (fname, old, text.count(old))
    if fname.endswith(".h"):                                      # a header: every source is compiled again, in a directory of its own
        top = src.parent / ("oracle_h%d" % k)
        top.mkdir()
        for f in os.listdir(src):
            if f.endswith((".c", ".h")) and not f.startswith(("mutant_", "smutant_")):
                shutil.copy(src / f, top / f)
        (top / fname).write_text(text.replace(old, new))
        so = top / "liborc_mutant.so"
        subprocess.run(cc + flags + ["-shared", "-o", str(so)] + srcs + ["-lm", "-lpthread"], cwd=top, check=True)
        return so
    changed = "smutant_%d_%s" % (k, fname)
    (src / changed).write_text(text.replace(old, new))
    so = src / ("liborc_smutant_%d.so" % k)
    subprocess.run(cc + flags + ["-c", changed, "-o", changed + ".o"], cwd=src, check=True)
    subprocess.run(cc + flags + ["-shared", "-o", str(so), changed + ".o"] + [f + ".o" for f in srcs if f != fname] + ["-lm", "-lpthread"],
                   cwd=src, check=True)
    return so


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_battery_notices_the_mutant(orc, true_shades, oracle_objects, mutant):
    title, fname, old, new, name = mutant
    lib = orc.load(str(build_mutant(oracle_objects, MUTANTS.index(mutant), fname, old, new)))
    ref = true_shades(name)
    rays = changed = 0
    for (label, bat, mask), want in zip(mutant_batteries(name), ref):
        osc = orc.OracleScene(bat[0].flatten(), lib=lib)
        got = shades(osc, bat)
        osc.close()
        bad = differ(got, want).any(axis=2)                       # [calls, rays]
        if mask is not None:
            bad = bad & mask[None, :]
        changed += int(bad.sum())
        rays += bad.size
    print(f"{title}: {changed} of {rays} (call, ray) answers of the {name} batteries differ")
    assert changed >= 1


# ---------------------------------------------------------------- float64, not through the oracle's estimator
class _Pod:
    def __init__(self, pod):
        self.pod = pod

    def to_pod(self):
        return self.pod


def f64_family(orc, family):
    """-> (largest relative deviation, rays kept, rays left out, rays on purpose) over the family's batteries without a ConvexVolume."""
    worst, kept, left, on_purpose = 0.0, 0, 0, 0
    for label, bat in list(sb.all_batteries(family)) + (list(sb.all_batteries("lobe_kinds")) if family == "lobe" else []):
        sc, cam, o, d, calls, c = bat
        if "margin" not in c:
            continue
        osc = orc.OracleScene(sc.flatten())
        brute = bf.Brute(sc)
        emission = [np.zeros(3) if isinstance(ob.material, Dielectric) else np.asarray(ob.material.emission, np.float64) for ob in sc.objects]
        margin = np.broadcast_to(c["margin"], (len(calls), len(o)))
        purpose = np.broadcast_to(c["purpose"], (len(calls), len(o)))
        for ci, (key, depth, samples, tmax) in enumerate(calls):
            if depth != 2:
                continue
            cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
            rows = []
            for i in range(len(o)):
                if purpose[ci, i]:
                    on_purpose += 1
                    continue
                if not margin[ci, i] > sb.MARGIN_BAR:
                    left += 1
                    continue
                r = osc.intersect(o[i], d[i], t_min=0.001, t_max=tmax, seed=SEED, pixel=key + i)
                if not r.hit:
                    rows.append((i, None, None, None, None, None))
                    continue
                nd, brdf, pdf = orc.scatter(_Pod(r.material), r.hitpoint[:], r.normal[:], r.frontface, d[i], seed=SEED, pixel=key + i)
                rows.append((i, np.float64(r.hitpoint[:]), np.float64(nd), np.float64(brdf), float(pdf), r))
            hitrows = [x for x in rows if x[1] is not None]
            obj, dist, robust = bf.closest(brute, np.array([x[1] for x in hitrows]), np.array([x[2] for x in hitrows]), 0.001, tmax)
            for (i, hp, nd, brdf, pdf, r), ob, rb_ in zip(hitrows, obj, robust):
                if not rb_:
                    left += 1
                    continue
                n = np.float64(r.normal[:])
                dot_term = min(max(abs(float(nd @ n)), 0.0), 1.0) if float(n @ n) > 0.0 else 1.0
                e0 = np.zeros(3) if r.material.kind == abi.MI_MAT_DIELECTRIC else np.float64(r.material.emission[:])
                want = e0 + dot_term * brdf * (emission[ob] if ob >= 0 else np.zeros(3)) / pdf
                got = np.float64(osc.shade(cam, o[i], d[i], seed=SEED, pixel=key + i, sample=0))
                dev = float(np.max(np.abs(got - want)) / max(float(np.max(np.abs(want))), 1e-30))
                assert dev < 1e-3, (label, ci, i, got, want)     # a gross difference is a wrong wall or lobe, not rounding
                worst = max(worst, dev)
                kept += 1
            for x in rows:
                if x[1] is None:                                  # the ray meets nothing: black
                    assert not np.any(osc.shade(cam, o[x[0]], d[x[0]], seed=SEED, pixel=key + x[0], sample=0)), (label, x[0])
                    kept += 1
        osc.close()
    return worst, kept, left, on_purpose


@pytest.mark.parametrize("family", ["lobe", "critical", "dot_term"])
def test_oracle_estimator_equals_float64_at_depth_2(orc, family):
    worst, kept, left, on_purpose = f64_family(orc, family)
    share = left / max(1, kept + left)
    print(f"{family}: {kept} rays kept, {left} left out ({share:.4f}), {on_purpose} on an edge on purpose; largest relative deviation {worst:.3e}, bar {F64_BAR:.3e}")
    assert kept >= 1000
    assert share <= F64_MAX_LEFT_OUT, share
    assert worst <= F64_BAR, worst


# ---------------------------------------------------------------- refusals
def test_shade_camera_checker_refuses_what_the_library_refuses():
    from cs397raytracingsp22_amd.tracing import check_shade_camera
    check_shade_camera(Camera(path_samples=1, max_trace_dist=float("inf")))
    check_shade_camera(Camera(path_samples=64, path_depth=0, max_trace_dist=0.0))
    with pytest.raises(ValueError, match="path_samples must be >= 1"):
        check_shade_camera(Camera(path_samples=0))
    with pytest.raises(ValueError, match="max_trace_dist must not be NaN"):
        check_shade_camera(Camera(max_trace_dist=float("nan")))
