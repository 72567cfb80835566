"""Hand-built rays and RNG keys aimed at the comparisons where Material::scatter and Scene::shade_ray decide: numpy only — no GPU, no oracle.

Every battery returns `(scene, camera, origins f32[n,3], dirs f32[n,3], calls, census)`: `calls` is a list of `(first_key, path_depth,
path_samples, max_trace_dist)` (the whole ray set is sent once per entry, ray i keyed first_key + i) and `census` counts, by a numpy-float32
restatement of the ONE expression in question in the reference's operation order, the rays that really sit on the edge the battery claims.
`census["purpose"]` marks the rays put on an edge on purpose and `census["margin"]` holds, per (call, ray), how far the decision is from
flipping (the float64 check of tests/test_shade_batteries_host.py keeps the rays whose margin is above MARGIN_BAR).

The colour room.  One probe object with the material under test sits at the origin inside a cube of 12 list Triangles, each with a
Lambertian of its own whose emission and albedo are distinct dyadic numbers.  With path_depth 2 the answer is
emission_probe + dot_term * brdf * E(wall) / pdf: which wall was hit, and dot_term.  With path_depth >= 3 the wall's own bounce starts at
the exact hitpoint, so the colour depends on every bit of new_d.

Exact geometry.  A Plane's normal reaches scatter raw (geometry.rs:478 multiplies by a signum, nothing is normalised); a Plane hit is always
a frontface hit (a ray along the signed normal is refused, geometry.rs:480).  The probe Triangle lies in y = 0 with the stored normal
(0,-1,0) exactly, so rays from above hit its BACK.  Directions are not unit: with n = (0,1,0) and d = (x,-c,0), cosv IS c.

RNG keys.  The stream (orc_rng.h) is restated below; `find_keys` searches [0, 2^26) for keys whose first gen01 is a wanted value or one
grid step (2^-23) beside it.  In a room without a ConvexVolume the first draw of a path is the scatter's own."""
import functools

import numpy as np

from cs397raytracingsp22_amd import (Camera, ConvexVolume, Dielectric, Isotropic, Lambertian, Metal, ParameterizedMaterial, Plane, Scene,
                                     Sphere, StaticMesh, Triangle, cgmath, objload)

from ray_batteries import F, INF, _QUIET, _pad, cross, cube_mesh, dot, f32, fclass, nxt, sphere_terms

SEED = 3
HALF = 4.0                                                  # the room's half width
MARGIN_BAR = 1.0e-4
DEPTHS = (2, 4)
M32 = 0xffffffff
STEP = F(2.0 ** -23)                                        # the grid of gen01


# ---------------------------------------------------------------- the RNG stream, restated (oracle/orc_rng.h)
def lowbias32(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def _rotl(x, k):
    return ((x << np.uint64(k)) | (x >> np.uint64(32 - k))) & M32


def rng_init(seed, pixel, sample=0):
    """-> (s0, s1) as uint64 arrays holding 32-bit values."""
    k0 = lowbias32(np.uint64(seed ^ 0x68e31da4))
    p0 = lowbias32((np.asarray(pixel, np.uint64) + k0) & M32)
    p1 = lowbias32(p0 ^ np.uint64(0xb5297a4d))
    s0 = lowbias32((p0 + np.uint64((sample * 0x9e3779b9) & M32)) & M32)
    s1 = lowbias32(p1 ^ np.uint64((sample * 0x85ebca6b) & M32))
    return s0, np.where((s0 | s1) == 0, np.uint64(1), s1)


def next_u32(s0, s1):
    """xoroshiro64**: -> (result, s0', s1')."""
    res = (_rotl((s0 * np.uint64(0x9e3779bb)) & M32, 5) * np.uint64(5)) & M32
    s1 = s1 ^ s0
    return res, _rotl(s0, 26) ^ s1 ^ ((s1 << np.uint64(9)) & M32), _rotl(s1, 13)


def rng_words(seed, pixel, n, sample=0):
    s0, s1 = rng_init(seed, np.uint64(pixel), sample)
    out = []
    for _ in range(n):
        r, s0, s1 = next_u32(s0, s1)
        out.append(int(r))
    return np.array(out, np.uint32)


def value1_2(bits):
    return (np.uint32(0x3f800000) | (np.asarray(bits, np.uint64) >> np.uint64(9)).astype(np.uint32)).view(np.float32)


def first_u(seed, keys):
    """The first gen01 of the streams (seed, key, 0): (0x3f800000 | bits >> 9) - 1."""
    s0, s1 = rng_init(seed, np.asarray(keys, np.uint64))
    return value1_2(next_u32(s0, s1)[0]) * F(1.0) + (F(0.0) - F(1.0))


class Rng:
    """One stream, draw by draw (for the census of the few rays whose scatter draws a vector)."""

    def __init__(self, seed, pixel):
        self.s0, self.s1 = rng_init(seed, np.uint64(pixel))

    def bits(self):
        r, self.s0, self.s1 = next_u32(self.s0, self.s1)
        return r

    def gen01(self):
        return value1_2(self.bits()) * F(1.0) + (F(0.0) - F(1.0))

    def gen_m11(self):
        return value1_2(self.bits()) * F(2.0) + (F(-1.0) - F(2.0))

    def rand_sphere_vec(self):                               # tracing.rs:71-79
        while True:
            v = f32([self.gen_m11(), self.gen_m11(), self.gen_m11()])
            if dot(v, v) <= F(1.0):
                return v


def _lowbias32_u32(x):
    """lowbias32 on a uint32 array, in place (uint32 products wrap)."""
    x ^= x >> np.uint32(16); x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15); x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


@functools.lru_cache(maxsize=None)
def find_keys(seed, mantissas, limit=1 << 26, want=8):
    """Keys in [0, limit) whose first gen01 is m * 2^-23 for m in `mantissas`: {m: [keys, ascending, at most `want`]}.  The first word of
    a stream depends on s0 = lowbias32(lowbias32(key + k0)) alone (sample 0)."""
    found = {m: [] for m in mantissas}
    wanted = np.array(sorted(mantissas), np.uint32)
    k0 = np.uint32(int(lowbias32(np.uint64(seed ^ 0x68e31da4))))
    chunk = 1 << 22
    for lo in range(0, limit, chunk):
        keys = np.arange(lo, lo + chunk, dtype=np.uint32)
        x = _lowbias32_u32(_lowbias32_u32(keys + k0))
        x *= np.uint32(0x9e3779bb)
        x = ((x << np.uint32(5)) | (x >> np.uint32(27))) * np.uint32(5)
        man = x >> np.uint32(9)
        for k in np.flatnonzero(np.isin(man, wanted)):
            lst = found[int(man[k])]
            if len(lst) < want:
                lst.append(int(keys[k]))
        if all(len(v) >= want for v in found.values()):
            break
    return found


def keys_around(targets, seed=SEED):
    """`targets`: values of u on the grid.  -> {u (float): [keys]} for each target and its two grid neighbours (those in [0, 1))."""
    ms = set()
    for t in targets:
        m = int(round(float(t) * 2 ** 23))
        ms |= {x for x in (m - 1, m, m + 1) if 0 <= x < 2 ** 23}
    found = find_keys(seed, tuple(sorted(ms)))
    return {m * 2.0 ** -23: list(v) for m, v in found.items()}


U_TARGETS = (0.0, 0.25, 0.5)


# ---------------------------------------------------------------- the colour room
def wall_material(k):
    return Lambertian(albedo=(0.5, 0.25 + k / 64.0, 0.75 - k / 32.0), emission=((k + 1) / 16.0, (12 - k) / 16.0, ((5 * k) % 13 + 1) / 16.0))


def walls(material_of=wall_material):
    p = cube_mesh(-HALF, HALF).positions.reshape(-1, 3, 3)
    return [Triangle(tuple(map(float, t[0])), tuple(map(float, t[1])), tuple(map(float, t[2])), material_of(k)) for k, t in enumerate(p)]


PROBE_TRI = ((-2.0, 0.0, -2.0), (2.0, 0.0, -2.0), (0.0, 0.0, 2.0))       # e1 x e2 = (0,-16,0): the stored normal is (0,-1,0) exactly
PROBE_SPHERE = ((0.0, -1.0, 0.0), 1.0)                                   # its pole is the origin
KINDS = ("plane", "triangle", "sphere", "mesh")


def probe_quad():
    """A two-triangle quad through the origin, tilted (a flat one is never entered, geometry.rs:65); its vertex normals are (0,1,0), and the
    mesh normal is interpolated from those."""
    pos = np.float32([[-2, 0.5, -2], [2, 0.5, -2], [2, -0.5, 2], [-2, -0.5, 2]])
    return objload.Mesh(pos, np.float32([[0, 1, 0]] * 4), np.float32([[0, 0], [1, 0], [1, 1], [0, 1]]), np.uint32([0, 1, 2, 0, 2, 3]))


def probe(kind, m, normal=(0.0, 1.0, 0.0), tri=PROBE_TRI):
    if kind == "plane":
        return Plane((0.0, 0.0, 0.0), tuple(float(x) for x in normal), m)
    if kind == "triangle":
        return Triangle(*[tuple(float(x) for x in v) for v in tri], m)
    if kind == "sphere":
        return Sphere(*PROBE_SPHERE, m)
    if kind == "mesh":
        return StaticMesh(probe_quad(), m, [None] * 5, cgmath.identity())
    raise KeyError(kind)


KIND_ORDER = (Triangle, Sphere, Plane, ConvexVolume, StaticMesh)


def room(probe_objects, material_of=wall_material):
    """The probe objects and the 12 walls, listed in the kernels' kind order (Triangles, Spheres, Planes, volumes, meshes): a scatter
    off a degenerate normal makes a NaN ray, whose "hit" at a NaN distance is the first one in evaluation order, and list order and kind
    order have to coincide for the kernels to agree with the reference there.  `scene.probe_index` is the first
    probe object's index: 0 for a Triangle, 12 for the other kinds."""
    probes = sorted(probe_objects, key=lambda ob: KIND_ORDER.index(type(ob)))
    tris = [ob for ob in probes if isinstance(ob, Triangle)]
    sc = Scene(Camera(), tris + walls(material_of) + [ob for ob in probes if not isinstance(ob, Triangle)])
    sc.probe_index = sc.objects.index(probe_objects[0])
    return sc


def tri_normal(tri):
    """geometry.rs:449 normalize(e1 x e2) = c * (1 / |c|)."""
    a = f32(tri[0])
    c = cross(f32(tri[1]) - a, f32(tri[2]) - a)
    with np.errstate(**_QUIET):
        return (c * (F(1.0) / np.sqrt(dot(c, c)))).astype(np.float32)


def facing(kind, o, d, normal=(0.0, 1.0, 0.0), tri=PROBE_TRI):
    """The probe's hit as RayHit::new leaves it (tracing.rs:121-126), restated: (normal facing the ray f32[n,3], frontface[n], hit[n]).
    For the mesh the normal is the nominal (0, +-1, 0): its chain (barycentric interpolation, two normalisations) is not restated."""
    o, d = f32(o), f32(d)
    n = len(o)
    with np.errstate(**_QUIET):
        if kind == "plane":                                                       # geometry.rs:476-481
            nrm = np.broadcast_to(f32(normal), (n, 3))
            od = dot(o, nrm)
            sg = np.where(np.isnan(od), od, np.where(np.signbit(od), F(-1.0), F(1.0))).astype(np.float32)
            ns = (nrm * sg[:, None]).astype(np.float32)
            hit = dot(d, ns) < 0
        elif kind == "triangle":
            ns = np.broadcast_to(tri_normal(tri), (n, 3))
            hit = np.ones(n, bool)
        elif kind == "sphere":                                                    # geometry.rs:397-411
            T = sphere_terms(o, d, *PROBE_SPHERE)
            t = np.where(T["t1"] >= F(0.001), T["t1"], T["t2"])
            hit = (T["disc"] >= 0) & (t >= F(0.001))
            v = (o + d * t[:, None]) - f32(PROBE_SPHERE[0])
            ns = (v * (F(1.0) / np.sqrt(dot(v, v)))[:, None]).astype(np.float32)
        else:
            ns = np.broadcast_to(f32([0.0, 1.0, 0.0]), (n, 3))
            hit = np.ones(n, bool)
        ff = dot(ns, d) < 0                                                       # tracing.rs:122
        nf = np.where(ff[:, None], ns, -ns).astype(np.float32)
    return nf, ff, hit


def fresnel(d, n, ir):
    """tracing.rs:58-62."""
    with np.errstate(**_QUIET):
        q = (F(ir) - F(1.0)) / (F(ir) + F(1.0))
        r0 = q * q
        a = F(1.0) - np.abs(dot(d, n))
        a2 = a * a
        a4 = a2 * a2
        return (r0 + (F(1.0) - r0) * (a * a4)).astype(np.float32)


def reflect(d, n):
    """tracing.rs:54-56  v - 2.0 * v.dot(n) * n."""
    with np.errstate(**_QUIET):
        return (f32(d) - f32(n) * (F(2.0) * dot(d, n))[..., None]).astype(np.float32)


def ulps_eq(a, b):
    """approx::ulps_eq!, f32 defaults: epsilon = f32::EPSILON, max_ulps = 4."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(**_QUIET):
        close = np.abs(a - b) <= F(1.1920929e-07)
        signs = (a < 0) != (b < 0)
        ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return close | (~signs & (ulps <= 4))


def rotation_branch(nf):
    """Which branch of Basis3::between_vectors(unit_y, n) a hit normal takes: 'identity' | 'pi' | 'general' per row."""
    nf = f32(nf).reshape(-1, 3)
    with np.errstate(**_QUIET):
        kc = nf[:, 1].copy()                                                       # (0 * x + 1 * y) + 0 * z
        k = np.sqrt(F(1.0) * dot(nf, nf))
        ident = ulps_eq(kc, np.full_like(kc, 1.0))
        pi = ~ident & ulps_eq(kc / k, np.full_like(kc, -1.0))
    out = np.full(len(nf), "general", dtype=object)
    out[ident] = "identity"
    out[pi] = "pi"
    return out


# ---------------------------------------------------------------- rays
def aimed(dirs, tag="bulk"):
    """Rays that reach the origin at t = 1: o = -d."""
    return [(tuple(-float(x) for x in d), tuple(float(x) for x in d), tag) for d in dirs]


def bulk_dirs(both_sides=True):
    """A fan of directions away from every edge: elevations c = 1/8 .. 7/8, four azimuths."""
    out = []
    for c in (0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 0.9375):
        for ax, az in ((1.0, 0.0), (0.0, 1.0), (-0.75, 0.5), (0.5, -0.75), (-0.625, -0.375)):
            x = float(np.sqrt(1.0 - c * c))
            out.append((x * ax, -c, x * az))
            if both_sides:
                out.append((x * ax, c, x * az))
    out += [(0.0, -1.0, 0.0), (0.0, -0.5, 0.0), (0.0, -2.0, 0.0)]
    return out


def _finish(P):
    P = _pad(P)
    o = f32([p[0] for p in P]).reshape(-1, 3)
    d = f32([p[1] for p in P]).reshape(-1, 3)
    purpose = np.array([p[2] != "bulk" for p in P])
    return o, d, purpose


def depth_calls(keys=(0,), depths=DEPTHS, samples=1, tmax=INF):
    return [(int(k), dp, samples, tmax) for k in keys for dp in depths]


def u_of_calls(calls, n):
    """first gen01 per (call, ray)."""
    return np.stack([first_u(SEED, np.arange(c[0], c[0] + n, dtype=np.uint64)) for c in calls])


# ---------------------------------------------------------------- critical angle
CRITICAL_IORS = (1.25, 1.5, 2.0, 4.0, 8.0, 3.0, 5.0, 1.125, 16.0, 0.8, 0.5, 0.125)


def critical_battery(ior=1.5, kind="triangle"):
    """Dielectric: `eta * sqrtf(1 - cosv^2) > 1.0f` (materials.rs:81) at equality.  For each side of the probe on which eta > 1 (the
    Triangle's back for ior > 1; the front of any probe for ior < 1) c sweeps +-40 consecutive floats around sqrt(1 - 1/eta^2); c in
    {1, nextafter(1, 2), 1.5, 4} exercises the fminf(.., 1) clamps (materials.rs:81, tracing.rs:65)."""
    m = Dielectric(ior)
    m.emission = (0.5, 0.25, 0.125)                                                # Material::emission of a Dielectric is zero (:102): never seen
    sc = room([probe(kind, m)])
    P = aimed(bulk_dirs())
    for sgn, front in ((-1.0, kind != "triangle"), (1.0, True)):                 # from above, from below
        eta = float(F(1.0) / F(ior)) if front else float(F(ior))
        if kind == "sphere" and sgn > 0:
            continue                                                               # from below the ray enters the sphere elsewhere
        if eta > 1.0:
            c0 = F(np.sqrt(1.0 - 1.0 / (eta * eta)))
            cs = [c0]
            for _ in range(40):
                cs = [nxt(cs[0], 0)] + cs + [nxt(cs[-1], 2)]
            P += aimed([(float(F(np.sqrt(max(0.0, 1.0 - float(c) ** 2)))), sgn * float(c), 0.0) for c in cs], "edge")
        P += aimed([(0.5, sgn * float(c), 0.0) for c in (F(1.0), nxt(1, 2), F(1.5), F(4.0))], "clamp")
    if kind == "sphere":                                                           # the equator: normal (-1, 0, 0)
        P += [((-3.0, -1.0, 0.0), (1.0, 0.0, 0.0), "bulk"), ((-3.0, -1.0, 0.0), (2.0, 0.0, 0.0), "bulk"), ((-3.0, -1.0, 0.25), (1.0, 0.0, 0.0), "bulk")]
    o, d, purpose = _finish(P)
    nf, ff, hit = facing(kind, o, d)
    with np.errstate(**_QUIET):
        eta = np.where(ff, F(1.0) / F(ior), F(ior)).astype(np.float32)          # :80
        cosv_raw = -dot(d, nf)
        cosv = np.minimum(cosv_raw, F(1.0))
        prod = (eta * np.sqrt(F(1.0) - cosv * cosv)).astype(np.float32)         # :81
    fr = fresnel(d, nf, ior)
    calls = depth_calls((0, 7000))
    u = u_of_calls(calls, len(o))
    crit = prod > F(1.0)
    with np.errstate(**_QUIET):
        margin = np.where(crit[None, :], np.abs(prod - F(1.0))[None, :], np.minimum(np.abs(prod - F(1.0))[None, :], np.abs(u - fr[None, :])))
    margin = np.where(np.isnan(margin), 0.0, margin)
    census = {"rays": len(o), "ior": ior, "kind": kind, "exact": kind != "mesh", "purpose": purpose, "margin": margin,
              "product == 1": int((hit & (prod == 1)).sum()), "product > 1": int((hit & (prod > 1)).sum()), "product < 1": int((hit & (prod < 1)).sum()),
              "cosv > 1 (the clamp is active)": int((hit & (cosv_raw > 1)).sum()), "cosv == 1": int((hit & (cosv_raw == 1)).sum()),
              "frontface (eta = 1 / ior)": int((hit & ff).sum()), "backface (eta = ior)": int((hit & ~ff).sum())}
    return sc, Camera(), o, d, calls, census


# ---------------------------------------------------------------- the Fresnel draw
def fresnel_draw_battery(ior=3.0, kind="plane"):
    """Dielectric at normal incidence, d = (0,-1,0): fresnel_factor = r0 exactly ((ior - 1) / (ior + 1))^2 — 0.25 for ior 3, 0 for ior 1
    (always refracts, even at u == 0), 1 for ior 0 (never refracts) — and grazing rays (d . n == 0: the factor is r0 + (1 - r0)).  Each key
    whose first draw is 0, 0.25 or 0.5 or a grid neighbour is a call of its own: ray 0 of that call draws it."""
    m = Dielectric(ior)
    m.emission = (0.5, 0.25, 0.125)
    sc = room([probe(kind, m)])
    P = aimed([(0.0, -1.0, 0.0)], "edge") + aimed(bulk_dirs())
    P += aimed([(0.0, -1.0, 0.0)] * 8, "bulk")
    # grazing: in the plane y = 0 towards the probe's surface (a Plane is missed, dd == 0; a Triangle has g == 0) — and one ulp off it
    P += [((-1.0, 0.0, 0.0), (1.0, 0.0, 0.0), "graze"), ((-1.0, float(nxt(0, 1)), 0.0), (1.0, -float(nxt(0, 1)), 0.0), "graze"),
          ((-1.0, 2.0 ** -100, 0.0), (1.0, -2.0 ** -100, 0.0), "graze"), ((-1.0, 2.0 ** -24, 0.0), (1.0, -2.0 ** -24, 0.0), "graze")]
    o, d, purpose = _finish(P)
    purpose[:] = False
    nf, ff, hit = facing(kind, o, d)
    fr = fresnel(d, nf, ior)
    keys = keys_around(U_TARGETS)
    calls = depth_calls(sorted(k for v in keys.values() for k in v[:2]) + [0])
    u = u_of_calls(calls, len(o))
    with np.errstate(**_QUIET):
        margin = np.abs(u - fr[None, :])
        graze = hit & (np.abs(dot(d, nf)) < F(2.0 ** -20))
    margin = np.where(np.isnan(margin), 0.0, margin)
    h = hit[None, :]
    census = {"rays": len(o), "calls": len(calls), "ior": ior, "kind": kind, "exact": kind != "mesh", "purpose": np.broadcast_to(purpose, u.shape) | (margin <= 2 * STEP),
              "margin": margin,
              "(ray, call): u < fresnel_factor": int((h & (u < fr)).sum()), "(ray, call): u == fresnel_factor": int((h & (u == fr)).sum()),
              "(ray, call): u > fresnel_factor": int((h & (u > fr)).sum()),
              "(ray, call): u one step below fresnel_factor": int((h & (u + STEP == fr)).sum()),
              "(ray, call): u one step above fresnel_factor": int((h & (u - STEP == fr)).sum()),
              "(ray, call): u == 0": int((h & (u == 0)).sum()),
              "fresnel_factor of the normal ray": float(fr[0]), "grazing rays (|d . n| < 2^-20)": int(graze.sum()),
              "grazing rays with fresnel_factor == 1": int((graze & (fr == 1)).sum())}
    return sc, Camera(), o, d, calls, census


# ---------------------------------------------------------------- the lobe choice
LOBE_VARIANTS = [(1.0, 0.75), (1.0, 0.5), (1.0, 1.0), (1.0, 0.0), (0.0, 0.5), (0.5, 0.5), (2.0, 0.5), (1.0, -0.5), (1.0, 1.5)]   # (roughness, metallic)


def lobe_battery(roughness=1.0, metallic=0.75, kind="plane"):
    """ParameterizedMaterial: `u < k_d` (materials.rs:120), k_d = (1 - fresnel * (1 - roughness)) * (1 - metallic).  roughness 1 makes
    k_s = 0 and k_d = 1 - metallic exactly: 0.25 / 0.5 against keys whose u is that value or a grid neighbour; metallic 1 gives k_d = 0
    (never diffuse, even at u == 0) and metallic 0 gives 1."""
    m = ParameterizedMaterial(albedo=(0.75, 0.5, 0.25), emission=(0.0625, 0.03125, 0.125), roughness=roughness, metallic=metallic)
    sc = room([probe(kind, m)])
    P = aimed([(0.0, -1.0, 0.0)], "edge") + aimed(bulk_dirs())
    if kind == "sphere":
        P += [((-3.0, -1.0, 0.0), (1.0, 0.0, 0.0), "bulk"), ((-3.0, -1.0, 0.25), (1.0, 0.0, 0.0), "bulk")]
    o, d, purpose = _finish(P)
    purpose[:] = False
    nf, ff, hit = facing(kind, o, d)
    with np.errstate(**_QUIET):
        k_s = fresnel(d, nf, 1.5) * (F(1.0) - F(roughness))                       # :116-117
        k_d = ((F(1.0) - k_s) * (F(1.0) - F(metallic))).astype(np.float32)      # :118
    keys = keys_around(U_TARGETS)
    calls = depth_calls(sorted(k for v in keys.values() for k in v[:2]) + [0])
    u = u_of_calls(calls, len(o))
    with np.errstate(**_QUIET):
        margin = np.abs(u - k_d[None, :])
    h = hit[None, :]
    diffuse = h & (u < k_d)
    census = {"rays": len(o), "calls": len(calls), "roughness": roughness, "metallic": metallic, "kind": kind, "exact": kind != "mesh",
              "purpose": np.broadcast_to(purpose, u.shape) | (margin <= 2 * STEP), "margin": margin,
              "(ray, call): u < k_d": int((h & (u < k_d)).sum()), "(ray, call): u == k_d": int((h & (u == k_d)).sum()),
              "(ray, call): u > k_d": int((h & (u > k_d)).sum()),
              "(ray, call): u one step below k_d": int((h & (u + STEP == k_d)).sum()), "(ray, call): u one step above k_d": int((h & (u - STEP == k_d)).sum()),
              "(ray, call): u == 0": int((h & (u == 0)).sum()),
              "(ray, call): diffuse lobe": int(diffuse.sum()), "(ray, call): specular lobe": int((h & ~diffuse).sum()),
              "k_d of the normal ray": float(k_d[0])}
    return sc, Camera(), o, d, calls, census


# ---------------------------------------------------------------- sample_hemisphere's rotation
def _search_scalar(fn, lo, hi, want, n=20000):
    """The first x on a grid of [lo, hi] at which fn(x) is each value of `want`: {value: x}."""
    out = {}
    for x in np.linspace(lo, hi, n):
        v = fn(float(x))
        if v in want and v not in out:
            out[v] = float(x)
            if len(out) == len(want):
                break
    return out


def _ulps_below_one(y):
    return int(F(1.0).view(np.int32)) - int(np.abs(F(y)).view(np.int32))


@functools.lru_cache(maxsize=None)
def plane_normals():
    """The rotation battery's Plane normals (hit from above and from below: n and -n reach between_vectors)."""
    N = []
    for k in range(9):
        y = 1.0 - k * 2.0 ** -24
        N += [(0.0, y, 0.0), (0.0, -y, 0.0), (2.0 ** -10, y, 0.0), (0.0, -y, 2.0 ** -10), (-(2.0 ** -11), y, 2.0 ** -12)]
    for k in range(1, 9):
        y = 1.0 + k * 2.0 ** -23
        N += [(0.0, y, 0.0), (2.0 ** -10, y, 0.0)]
    N += [(0.0, 0.5, 0.0), (0.0, 2.0, 0.0), (0.0, 2.0 ** -60, 0.0), (0.0, 2.0 ** -70, 0.0), (0.0, 2.0 ** -80, 0.0), (0.0, 0.0, 0.0),
          (0.25, 0.5, 0.125), (2.0 ** -61, 2.0 ** -60, 0.0)]

    # a small x so that n.y / |n| lands 0..8 ulps from -1 for the ray that comes from below (the pi-rotation test).  With |n.y| = 1 only
    # even counts occur (|n| moves in steps of 2^-23 above 1), so the search runs over several lengths of n.y; every count 0..8 is found.
    found = {}
    for y in (1.0, 1.5, 1.75, 1.25, 3.0, 0.75, 0.875):
        def ratio_ulps(e):
            n = f32([e, y, 0.0])
            with np.errstate(**_QUIET):
                return _ulps_below_one(n[1] / np.sqrt(F(1.0) * dot(n, n)))
        for k, e in _search_scalar(ratio_ulps, 0.0, y * 2.0 ** -10, set(range(9)) - set(found), n=6000).items():
            found[k] = (e, y, 0.0)
    N += [n for _, n in sorted(found.items())]
    return N


@functools.lru_cache(maxsize=None)
def tilted_triangles():
    """List Triangles through the origin, tilted about x so that normalize(e1 x e2).y lands 0..8 ulps from -1 (stored), each also with
    the winding reversed (stored normal near +1): found by search, the normal restated by tri_normal."""
    def tri_of(h, w, flip=False):
        a, b, c = (-w, 0.5 * h, -2.0), (w, 0.5 * h, -2.0), (0.0, -0.5 * h, 2.0)          # y = -h z / 4 through the origin; e1 x e2 = (0, -8 w, -2 w h)
        return (a, c, b) if flip else (a, b, c)

    def ratio_ulps(h, w):
        n = tri_normal(tri_of(h, w))
        with np.errstate(**_QUIET):
            return _ulps_below_one(n[1] / np.sqrt(F(1.0) * dot(n, n)))
    # with w = 2 the cross product's length sits just above 16 and 1 / |c| moves in steps of two ulps of n.y: only even counts occur.
    # Other half widths put |c| elsewhere in its binade; every count 0..8 is found for both tests.
    found_y, found_r = {}, {}
    hs = np.linspace(0.0, 0.02, 20000)
    one = int(F(1.0).view(np.int32))
    for w in (2.0, 1.5, 1.75, 1.25, 1.875, 1.625):
        A, B, C = (f32(np.stack([np.full_like(hs, x), sy * 0.5 * hs, np.full_like(hs, z)], axis=-1)) for x, sy, z in ((-w, 1, -2.0), (w, 1, -2.0), (0.0, -1, 2.0)))
        c = cross(B - A, C - A)                                                     # tri_normal, for every h at once
        with np.errstate(**_QUIET):
            n = (c * (F(1.0) / np.sqrt(dot(c, c)))[:, None]).astype(np.float32)
            ratio = (n[:, 1] / np.sqrt(F(1.0) * dot(n, n))).astype(np.float32)
        for vals, found in ((n[:, 1], found_y), (ratio, found_r)):
            ulps = one - np.abs(vals).view(np.int32)
            for k in set(range(9)) - set(found):
                at = np.flatnonzero(ulps == k)
                if len(at):
                    found[k] = (float(hs[at[0]]), w)
    for k, (h, w) in list(found_y.items()) + list(found_r.items()):                 # the scalar restatement agrees with the search
        assert k in (_ulps_below_one(tri_normal(tri_of(h, w))[1]), ratio_ulps(h, w)), (k, h, w)
    out = []
    for h, w in sorted(set(found_y.values()) | set(found_r.values())):
        out += [tri_of(h, w), tri_of(h, w, True)]
    return out


def rotation_battery(form="plane", index=0):
    """Lambertian: Basis3::between_vectors(unit_y, n) (materials.rs:176) at the ulps_eq thresholds — identity (n.y within 4 ulps of 1),
    pi rotation (n.y / |n| within 4 ulps of -1), general.  `form` "plane": Plane normals plane_normals()[index], the normal reaches
    between_vectors raw; "triangle": list Triangles tilted_triangles()[index] (the kernel reads their rotation from a table the host
    computed).  Rays come from above and from below, so both n and -n are presented."""
    m = Lambertian(albedo=(0.75, 0.5, 0.25), emission=(0.0625, 0.03125, 0.125))
    if form == "plane":
        normal = plane_normals()[index]
        sc = room([probe("plane", m, normal=normal)])
        tri = None
    else:
        tri = tilted_triangles()[index]
        normal = tuple(float(x) for x in tri_normal(tri))
        sc = room([probe("triangle", m, tri=tri)])
    dirs = [(0.0, -1.0, 0.0), (0.0, 1.0, 0.0)] + [dd for dd in bulk_dirs() if abs(dd[1]) >= 0.25]
    o, d, purpose = _finish(aimed(dirs, "edge"))
    nf, ff, hit = facing(form, o, d, normal=normal, tri=tri or PROBE_TRI)
    br = rotation_branch(nf)
    with np.errstate(**_QUIET):
        ratio = nf[:, 1] / np.sqrt(F(1.0) * dot(nf, nf))
    up, down = hit & (nf[:, 1] > 0.5) & (nf[:, 1] < 1.5), hit & (ratio < -0.5)
    census = {"rays": len(o), "form": form, "normal": normal,
              "n.y ulps from 1 (identity test)": abs(_ulps_below_one(nf[up][0, 1])) if up.any() else None,
              "n.y / |n| ulps from -1 (pi test)": abs(_ulps_below_one(ratio[down][0])) if down.any() else None, "purpose": purpose, "probe hits": int(hit.sum()), "branch": np.where(hit, br, "miss"), "up": up, "down": down,
              "identity": int((hit & (br == "identity")).sum()), "pi": int((hit & (br == "pi")).sum()), "general": int((hit & (br == "general")).sum()),
              "rot table (list Triangle)": int(form == "triangle")}
    return sc, Camera(), o, d, depth_calls((0,)), census


def rotation_count(form):
    return len(plane_normals() if form == "plane" else tilted_triangles())


# ---------------------------------------------------------------- dot_term
DOT_VARIANTS = ["metal0", "metal1", "metal2", "volume", "tiny_normal", "zero_normal"]


def dot_term_battery(variant="metal0", kind="plane"):
    """tracing.rs:313 `dot_term = if mag2(n) > 0 { |new_d . n|.clamp(0, 1) } else { 1 }`.  metal0: Metal of roughness 0 with |d| in
    {2^-20, 0.5, 2, 4, 2^20} (|new_d . n| = |d . n|: the clamp at 1 is active or not) and d parallel to the surface up to one ulp;
    metal1 / metal2: roughness 1 and 2, whose new_d may enter the object; volume: an Isotropic ConvexVolume of density 1e3 (the hit normal is
    zero); tiny_normal: a Plane whose normal (0, 2^-80, 0) has mag2 == 0 in f32 (and 2^-70: a denormal mag2 > 0); zero_normal: the Plane
    with the zero normal, which no ray hits (d . n == 0 is refused, geometry.rs:480)."""
    P = []
    normal = (0.0, 1.0, 0.0)
    if variant.startswith("metal"):
        rough = float(variant[5:])
        m = Metal(albedo=(0.75, 0.5, 0.25), emission=(0.0625, 0.03125, 0.125), roughness=rough)
        objs = [probe(kind, m)]
        P += aimed(bulk_dirs())
        for s in (2.0 ** -20, 0.5, 2.0, 4.0, 2.0 ** 20):
            P += aimed([(0.5 * s, -0.5 * s, 0.25 * s), (0.0, -s, 0.0), (0.75 * s, -0.25 * s, 0.0)], "edge")
        if kind != "sphere":
            for e in (2.0 ** -24, 2.0 ** -100, float(nxt(0, 1))):
                P.append(((-1.0, e, 0.0), (1.0, -e, 0.0), "edge"))
        else:                                                                      # the equator: normal (-1, 0, 0); |d . n| = |d.x|
            for s in (0.5, 1.0, 2.0, 4.0):
                P += [((-3.0, -1.0, 0.0), (s, 0.0, 0.0), "edge"), ((-3.0, -1.0, 0.25), (s, 0.0, 0.0), "edge")]
    elif variant == "volume":
        objs = [ConvexVolume(Sphere(*PROBE_SPHERE, wall_material(0)), Isotropic(albedo=(0.75, 0.5, 0.25), emission=(0.0625, 0.03125, 0.125)), 1.0e3)]
        kind = "sphere"
        P += aimed(bulk_dirs(both_sides=False), "edge")
    else:
        m = Lambertian(albedo=(0.75, 0.5, 0.25), emission=(0.0625, 0.03125, 0.125))
        normal = (0.0, 0.0, 0.0) if variant == "zero_normal" else (0.0, 2.0 ** -80, 0.0)
        objs = [probe("plane", m, normal=normal)]
        if variant == "tiny_normal":
            objs.append(Plane((0.0, -1.0, 0.0), (0.0, 2.0 ** -70, 0.0), Metal(albedo=(0.5, 0.5, 0.75), emission=(0.125, 0.0625, 0.03125), roughness=0.0)))
        kind = "plane"
        P += aimed(bulk_dirs(), "edge")
    sc = room(objs)
    o, d, purpose = _finish(P)
    calls = depth_calls((0,))
    nf, ff, hit = facing(kind, o, d, normal=normal)
    with np.errstate(**_QUIET):
        n2 = dot(nf, nf)
    census = {"rays": len(o), "variant": variant, "kind": kind, "exact": kind != "mesh", "purpose": purpose}
    if variant.startswith("metal"):
        nd = reflect(d, nf)
        if rough != 0.0:
            v = np.stack([Rng(SEED, i).rand_sphere_vec() for i in range(len(o))])
            nd = (nd + v * F(rough)).astype(np.float32)
        with np.errstate(**_QUIET):
            dn = dot(nd, nf)
        census.update({"clamp active (|new_d . n| > 1)": int((hit & (np.abs(dn) > 1)).sum()), "|new_d . n| <= 1": int((hit & (np.abs(dn) <= 1)).sum()),
                       "new_d . n > 0 (leaves the surface)": int((hit & (dn > 0)).sum()), "new_d . n < 0 (enters the object)": int((hit & (dn < 0)).sum()),
                       "|d . n| below 2^-20 (parallel up to an ulp)": int((hit & (np.abs(dot(d, nf)) < F(2.0 ** -20))).sum()),
                       "mag2(n) > 0": int((hit & (n2 > 0)).sum())})
        with np.errstate(**_QUIET):
            margin = np.abs(np.abs(dn) - F(1.0))
        census["margin"] = np.where(np.isnan(margin), 0.0, margin)[None, :]
    elif variant == "volume":
        census.update({"rays into the dense volume (hit normal zero: the else arm)": int(hit.sum())})
    else:
        census.update({"probe hits": int(hit.sum()), "mag2(n) == 0 on a hit (the else arm)": int((hit & (n2 == 0)).sum()),
                       "mag2(n) class": sorted(set(fclass(n2)))})
    return sc, Camera(), o, d, calls, census


# ---------------------------------------------------------------- recursion depth, path_samples, max_trace_dist
DEPTH_CALLS = ([(0, dp, 1, INF) for dp in (0, 1, 2, 63, 64)] + [(1000, 6, 2, INF), (2000, 6, 3, INF), (3000, 2, 64, INF)]
               + [(4000, 6, 1, tm) for tm in (HALF, float(nxt(HALF, 0)), float(nxt(HALF, 8)), 2 * HALF, float(nxt(2 * HALF, 0)))])


def mirror_material(k):
    return Metal(albedo=(1.0 - 2.0 ** -6,) * 3, emission=((k + 1) * 2.0 ** -10, (12 - k) * 2.0 ** -10, 2.0 ** -9), roughness=0.0)


def depth_battery():
    """A closed room of mirrors (Metal, roughness 0, albedo 1 - 2^-6, small emission): no path escapes, so the recursion ends only at
    path_depth (tracing.rs:301) or at max_trace_dist (:305).  Axis rays from the centre meet a wall at t = HALF exactly and then cross the
    whole room (t = 2 HALF) for ever; the census counts their shade_ray levels that intersect, without the oracle."""
    sc = Scene(Camera(), walls(mirror_material))
    axes = [(1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 0.0, -1.0)]
    P = [((0.0, 0.0, 0.0), a, "edge") for a in axes]
    P += [((0.25, -0.5, 0.125), tuple(float(x) for x in dd), "bulk") for dd in bulk_dirs()]
    P += [((0.25, 0.5, -1.0), a, "bulk") for a in axes]
    o, d, purpose = _finish(P)
    axis = np.all(o == 0, axis=1)

    def levels(depth, samples, tmax):                          # intersecting levels of one axis ray from the centre: 1 + S + S^2 + ...
        reach = 0 if depth == 0 else (1 if HALF > tmax else (min(depth, 2) if 2 * HALF > tmax else depth))
        return sum(samples ** l for l in range(reach))

    def hits(depth, tmax):                                     # the hits along one mirror path from the centre (every sample repeats it)
        return 0 if depth == 0 or HALF > tmax else (1 if 2 * HALF > tmax else depth)
    census = {"rays": len(o), "calls": len(DEPTH_CALLS), "purpose": purpose, "axis rays from the centre": int(axis.sum()),
              "segments of one axis ray, per call": [levels(dp, s, tm) for _, dp, s, tm in DEPTH_CALLS],
              "hits along one axis path, per call": [hits(dp, tm) for _, dp, s, tm in DEPTH_CALLS],
              "calls at path_depth 64": sum(1 for c in DEPTH_CALLS if c[1] == 64), "calls at path_depth 0": sum(1 for c in DEPTH_CALLS if c[1] == 0),
              "calls with path_samples > 1": sum(1 for c in DEPTH_CALLS if c[2] > 1),
              "calls whose max_trace_dist is a hit distance exactly": sum(1 for c in DEPTH_CALLS if c[3] in (HALF, 2 * HALF)),
              "calls whose max_trace_dist is one ulp below a hit distance": sum(1 for c in DEPTH_CALLS if c[3] in (float(nxt(HALF, 0)), float(nxt(2 * HALF, 0))))}
    return sc, Camera(), o, d, list(DEPTH_CALLS), census


# ---------------------------------------------------------------- non-finite material parameters
NONFINITE_VARIANTS = ["inf_emission_zero_albedo", "nan_albedo", "ior -1", "ior inf", "ior nan", "ior 2^-140", "nan_roughness_metal", "nan_roughness_param",
                      "inf_emission_probe"]


def nonfinite_battery(variant="nan_albedo"):
    """Material parameters nothing refuses: an emission of +inf on the walls against an albedo of 0 on the probe (0 * inf), a NaN albedo,
    ior in {-1, +inf, NaN, 2^-140}, a NaN roughness.  The bar is same_f32: equal, or NaN on both sides."""
    nan = float("nan")
    wm = wall_material
    em = (0.0625, 0.03125, 0.125)
    if variant == "inf_emission_zero_albedo":
        m = Lambertian(albedo=(0.0, 0.5, 0.0), emission=em)
        wm = lambda k: Lambertian(albedo=(0.5, 0.5, 0.5), emission=(INF, (k + 1) / 16.0, INF if k % 2 else 0.25))
    elif variant == "inf_emission_probe":
        m = Metal(albedo=(0.0, 0.5, 1.0), emission=(INF, -INF, 1.0), roughness=0.5)
    elif variant == "nan_albedo":
        m = Lambertian(albedo=(nan, 0.5, 0.25), emission=em)
    elif variant.startswith("ior"):
        m = Dielectric({"-1": -1.0, "inf": INF, "nan": nan, "2^-140": 2.0 ** -140}[variant.split()[1]])
    elif variant == "nan_roughness_metal":
        m = Metal(albedo=(0.75, 0.5, 0.25), emission=em, roughness=nan)
    else:
        m = ParameterizedMaterial(albedo=(0.75, 0.5, 0.25), emission=em, roughness=nan, metallic=0.5)
    sc = room([probe("triangle", m)], wm)
    o, d, purpose = _finish(aimed(bulk_dirs(), "edge"))
    pod = m.to_pod()
    vals = list(pod.albedo) + list(pod.emission) + [pod.roughness, pod.metallic, pod.idx_of_refraction]
    wvals = [x for k in range(12) for x in wm(k).emission]
    census = {"rays": len(o), "variant": variant, "purpose": purpose,
              "non-finite or denormal parameters of the probe or the walls": int(sum(1 for x in vals + wvals if fclass([x])[0] in ("inf", "nan", "denormal"))),
              "finite parameters outside the sane range (a negative ior)": int(pod.idx_of_refraction < 0)}
    return sc, Camera(), o, d, depth_calls((0,)), census


# ---------------------------------------------------------------- the list of everything
def all_batteries(family):
    """(label, battery) for every scene of a family."""
    if family == "critical":
        for ior in CRITICAL_IORS:
            yield f"critical ior {ior} triangle", critical_battery(ior, "triangle")
        for kind in ("plane", "sphere", "mesh"):
            for ior in (0.5, 2.0):
                yield f"critical ior {ior} {kind}", critical_battery(ior, kind)
    elif family == "fresnel":
        for ior in (3.0, 1.0, 0.0):
            for kind in ("plane", "triangle"):
                yield f"fresnel ior {ior} {kind}", fresnel_draw_battery(ior, kind)
    elif family == "lobe":
        for r, mt in LOBE_VARIANTS:
            yield f"lobe roughness {r} metallic {mt} plane", lobe_battery(r, mt, "plane")
    elif family == "lobe_kinds":
        for kind in ("triangle", "sphere", "mesh"):
            for r, mt in ((1.0, 0.5), (0.0, 0.75)):
                yield f"lobe roughness {r} metallic {mt} {kind}", lobe_battery(r, mt, kind)
    elif family == "rotation_plane":
        for i in range(rotation_count("plane")):
            yield f"rotation plane {i}", rotation_battery("plane", i)
    elif family == "rotation_triangle":
        for i in range(rotation_count("triangle")):
            yield f"rotation triangle {i}", rotation_battery("triangle", i)
    elif family == "dot_term":
        for v in DOT_VARIANTS:
            yield f"dot_term {v}", dot_term_battery(v)
        for kind in ("triangle", "sphere", "mesh"):
            for v in ("metal0", "metal1"):
                yield f"dot_term {v} {kind}", dot_term_battery(v, kind)
    elif family == "depth":
        yield "depth", depth_battery()
    elif family == "nonfinite":
        for v in NONFINITE_VARIANTS:
            yield f"nonfinite {v}", nonfinite_battery(v)
    else:
        raise KeyError(family)


FAMILIES = ["critical", "fresnel", "lobe", "lobe_kinds", "rotation_plane", "rotation_triangle", "dot_term", "depth", "nonfinite"]
MESH_PROBE_LABELS = ("critical ior 0.5 mesh", "critical ior 2.0 mesh", "lobe roughness 1.0 metallic 0.5 mesh", "lobe roughness 0.0 metallic 0.75 mesh",
                     "dot_term metal0 mesh", "dot_term metal1 mesh")
