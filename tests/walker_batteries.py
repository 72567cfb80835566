"""Ray tables aimed at the decision edges of the mesh walkers behind wf_main (wf_trav, the three wf_trav_i forms, wf_filter_f / wf_trav_f /
wf_replay): numpy only — no GPU, no oracle.  tests/test_walker_batteries_host.py checks the census, tests/test_gpu_walker_batteries.py
renders the tables with mi_render_rays in every walker mode and compares path signatures with the oracle's orc_shade_sig.

Geometry: a LATTICE MESH built here — a 12 x 12 height field over [-3, 3]^2 with seeded heights, a 6 x 6 second sheet above its middle and
a copy of triangle 0 at the end of the index list: 361 triangles, every coordinate a multiple of 2^-3 inside [-4, 4].  Every box plane of
every node of its tree is then a lattice number whatever the builder did, and the slab arithmetic of an axis-parallel ray from a lattice
origin is exact.  A leaf of the reference's tree holds one triangle (geometry.rs:190-217), so any two triangles lie in different leaves:
the two coincident ones (leaf 0 and the last leaf, on opposite sides of the root), and every pair that shares an edge.  Texcoords put
triangle k alone into texel k + 33 of a 32 x 16 index texture (ray_batteries.index_texture), so a colour names a triangle.

The rays are made in the lattice mesh's OBJECT space and mapped to world space by the mesh's transform, exactly (integer translations,
power-of-two scales, a mirror), as ray_batteries.mesh_battery does.  Which ray meets which edge is NOT assumed: `trace` restates
BVHNode::intersect (geometry.rs:94-119) with AABB::intersect (:52-79) and the IndexedTriangle test (:331-349) in f32 on the node boxes, links
and leaf contents decoded from the compiled scene (tests/test_scene_compile_host.py's Blob), along the reference's own depth-first order, and
the census counts what that walk met at the interior nodes BELOW the root.  Candidates are generated around a choice of such nodes; only
those the walk confirms are kept.

Kinds (the letters of the census):
  a   an axis-parallel ray lying in a face plane of an interior node below the root: (plane - o) * (1 / 0) = 0 * inf = NaN in the slab
  a-  the same rays with -0.0 for the zero components in WORLD space.  Transform3::transform_vector ends in `+ m[12 + row] * 0.0`, so what
      object space sees is -0.0 (1/d = -inf) only where the inverse's translation is negative as well and +0.0 everywhere else: the zero's
      sign changes on the way, per axis and per scene.  The restated walk gives the same answer for either sign (the host test asserts it)
  b   a ray with dyadic direction components ((1, 1, 0), (1, 2, -1), ...) through an edge or corner of such a node: t_in == t_out bit for bit,
      the box test's `tmax <= tmin` decides
  c   the entry distance of such a node equals, bit for bit, the hit found in its left sibling, which is the bound it is tested with (:113)
  d   max_trace_dist at a hit distance exactly, at its two f32 neighbours, and ending inside an interior box (three further calls)
  e   hits at a vertex, on an edge shared with another triangle that accepts the same distance, and in the coincident pair
  f   origins strictly inside such a node's box, and on one of its faces
  g   each ray of a, b, e, f again with d * 2^20 and d * 2^-20 (at 2^20 every distance is below shade_ray's t_min = 0.001: the root rejects)
  h   wave composition: eight table rows (536 entries; a wf_main block is 8 rows of a 32-pixel tile) of rays with a zero direction
      component, eight of rays without, eight alternating the two, eight in which only every 17th entry enters any root box
  i   two small tables for the `one` scene: exactly one entry enters the root box; none does"""
import numpy as np

from cs397raytracingsp22_amd import Camera, Lambertian, Metal, Scene, StaticMesh, cgmath, objload, scenes

import ray_batteries as rb

F = np.float32
WIDTH = 67                                  # ragged in 32-pixel tiles: every render has padded lanes
SEED = 5
FAR = float(2.0 ** 40)                      # max_trace_dist of the main call: the 2^-20 rays hit at distances up to 2^23
T_MIN = F(0.001)                            # shade_ray's t_min (tracing.rs:305)
TEX_W, TEX_H, TEXEL_OFFSET = 32, 16, 33
_QUIET = dict(over="ignore", under="ignore", invalid="ignore", divide="ignore")


# ---------------------------------------------------------------------------------------------- geometry
def lattice_triangles(seed=11):
    """[361, 3, 3] float64 corners, all multiples of 1/8"""
    rng = np.random.default_rng(seed)
    tris = []

    def sheet(n, x0, heights):
        for j in range(n):
            for i in range(n):
                p = lambda a, b: (x0 + 0.5 * a, float(heights[b, a]), x0 + 0.5 * b)        # noqa: E731
                p00, p10, p11, p01 = p(i, j), p(i + 1, j), p(i + 1, j + 1), p(i, j + 1)
                tris.append((p00, p11, p10))
                tris.append((p00, p01, p11))
    sheet(12, -3.0, rng.integers(-8, -1, (13, 13)) / 8.0)          # heights in [-1, -0.25]
    sheet(6, -1.5, rng.integers(8, 13, (7, 7)) / 8.0)              # the second sheet: heights in [1, 1.5]
    tris.append(tris[0])                                           # coincident with triangle 0, in the last leaf
    return np.array(tris, np.float64)


def texel_of_triangle(k):
    return (k + TEXEL_OFFSET) % TEX_W, (k + TEXEL_OFFSET) // TEX_W


def lattice_mesh():
    T = lattice_triangles()
    n = len(T)
    pos = T.reshape(-1, 3).astype(np.float32)
    nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    nrm = np.repeat(nrm / np.linalg.norm(nrm, axis=1, keepdims=True), 3, axis=0).astype(np.float32)
    uv = np.zeros((n, 3, 2), np.float32)
    for k in range(n):                                            # three distinct points well inside the triangle's own texel
        tx, ty = texel_of_triangle(k)
        for j, (a, b) in enumerate(((0.25, 0.25), (0.75, 0.25), (0.5, 0.75))):
            uv[k, j] = ((tx + a) / TEX_W, 1.0 - (ty + b) / TEX_H)
    return objload.Mesh(pos, nrm, uv.reshape(-1, 2), np.arange(3 * n, dtype=np.uint32), "lattice")


def one_triangle_mesh():
    """Its root is a leaf: never box-tested (geometry.rs:95).  Above both sheets."""
    pos = np.float32([[-0.5, 2.5, 0.0], [0.5, 2.5, 0.0], [0.0, 3.0, 0.5]])
    n = np.cross(pos[1] - pos[0], pos[2] - pos[0])
    return objload.Mesh(pos, np.float32([n / np.linalg.norm(n)] * 3), np.float32([[0, 0], [1, 0], [0, 1]]), np.uint32([0, 1, 2]), "one")


LATTICE = lattice_mesh()
N_TRIS = LATTICE.n_triangles
ONE_M = cgmath.mul(cgmath.from_translation((0.0, 2.0, 0.0)), cgmath.from_scale(0.5))      # into the Cornell box: [-1.5, 1.5] x [1.5, 2.75] x [-1.5, 1.5]
SCENES = ("one", "one-mirror", "one-emission") + tuple(f"multi-{t}" for t in sorted(rb.MESH_TRANSFORMS))


def scene(name, height):
    """-> (Scene, the lattice mesh's transform, its index in Scene.objects).  `multi` is one scene per transform of rb.MESH_TRANSFORMS (all
    four keep the scene bounded): the trees of two lattice meshes would not fit the paired walker's 40 KB, and MI_RT_WF_TRAV_LDS is
    silently ignored for trees that do not fit."""
    cam = Camera(path_depth=4, path_samples=1, aa_sample_count=1, screen_width=WIDTH, screen_height=height, max_trace_dist=FAR)
    if name.startswith("one"):
        M = ONE_M
        if name == "one":
            lat = StaticMesh(LATTICE, Lambertian(albedo=(0.6, 0.5, 0.4)), [None] * 5, M)
        elif name == "one-mirror":
            lat = StaticMesh(LATTICE, Metal(albedo=(0.9, 0.9, 0.9), roughness=0.0), [None] * 5, M)
        else:
            lat = StaticMesh(LATTICE, None, [None, rb.index_texture(TEX_W, TEX_H), None, None, None], M)
            cam.path_depth = 1
        return Scene(cam, scenes.cornell_walls() + [lat]), np.asarray(M, np.float64), 10
    M = rb.MESH_TRANSFORMS[name[len("multi-"):]]
    lat = StaticMesh(LATTICE, Lambertian(albedo=(0.6, 0.5, 0.4), emission=(0.5, 0.5, 0.5)), [None] * 5, M)
    objs = [lat, StaticMesh(one_triangle_mesh(), Lambertian(albedo=(0.3, 0.6, 0.3), emission=(0.25, 0.5, 0.25)), [None] * 5, M),
            StaticMesh(rb.quad_mesh(), Lambertian(albedo=(0.3, 0.3, 0.7)), [None] * 5, M), lat]
    return Scene(cam, objs), np.asarray(M, np.float64), 0


def to_world(M, o, d):
    """M * (o, 1), M * (d, 0) in f64, rounded once: exact for these matrices and lattice rays; the sign of a zero component is kept."""
    wo = (M[:3, :3] @ o.T.astype(np.float64)).T + M[:3, 3]
    wd = (M[:3, :3] @ d.T.astype(np.float64)).T
    wd = np.where((d == 0) & (wd == 0), np.copysign(0.0, d.astype(np.float64)), wd)
    return rb.f32(wo), rb.f32(wd)


def to_object(inv16, wo, wd):
    """Transform3::transform_point / transform_vector with the mesh's inv_transform (column-major 16 floats), restated in f32 in the
    reference's order: ((m0 x + m4 y) + m8 z) + m12 w, the point divided by its own w."""
    m = np.asarray(inv16, np.float32)
    with np.errstate(**_QUIET):
        def row(r, v, w):
            return ((m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + m[8 + r] * v[:, 2]) + m[12 + r] * F(w)
        iw = F(1.0) / row(3, wo, 1.0)
        o = np.stack([row(0, wo, 1.0) * iw, row(1, wo, 1.0) * iw, row(2, wo, 1.0) * iw], axis=1)
        d = np.stack([row(0, wd, 0.0), row(1, wd, 0.0), row(2, wd, 0.0)], axis=1)
    return rb.f32(o), rb.f32(d)


# ---------------------------------------------------------------------------------------------- the decoded tree and the restated walk
class Tree:
    """Node boxes, links and leaf contents of one mesh's reference tree as the scene compiler wrote them (a Blob of test_scene_compile_host.py):
    nodes in depth-first order, left before right; interior node j has its left child at j + 1 and its right child at end[j + 1]."""

    def __init__(self, blob, mesh=0):
        M = blob.meshes[mesh]
        nb, ne = int(M["node_begin"]), int(M["node_end"])
        self.lo, self.hi = blob.nodes[nb:ne, 0:3].copy(), blob.nodes[nb:ne, 4:7].copy()
        self.end = (blob.nodes_i[nb:ne, 3] - nb).astype(np.int64)
        self.tri = blob.nodes_i[nb:ne, 7].astype(np.int64)
        T = blob.tris[int(M["tri_begin"]):int(M["tri_begin"]) + int(M["n_tris"])]
        self.A, self.E1, self.E2 = T[:, 0:3].copy(), T[:, 4:7].copy(), T[:, 8:11].copy()       # {a, e1, e2}: the leaf contents
        self.n = ne - nb
        self.depth = np.zeros(self.n, np.int64)
        self.parent = np.full(self.n, -1, np.int64)
        for j in range(self.n):
            if self.tri[j] < 0:
                for c in (j + 1, int(self.end[j + 1])):
                    self.depth[c], self.parent[c] = self.depth[j] + 1, j
        self.inner = np.flatnonzero((self.tri < 0) & (self.depth >= 1))                       # interior nodes below the root


def _fmax(a, b):        # f32::max: the non-NaN operand
    return b if a != a else (a if b != b else max(a, b))


def _fmin(a, b):
    return b if a != a else (a if b != b else min(a, b))


class Walk:
    """The restated walk of every ray of (o, d) (object space, f32) through `tree`.  Everything that rounds is computed once, vectorised, in
    numpy float32 in the reference's operation order; the walk itself only compares."""

    def __init__(self, tree, o, d):
        self.tree, self.o, self.d = tree, rb.f32(o), rb.f32(d)
        inner = np.flatnonzero(tree.tri < 0)
        self.slot = np.full(tree.n, -1, np.int64)
        self.slot[inner] = np.arange(len(inner))
        with np.errstate(**_QUIET):
            inv = F(1.0) / self.d                                                             # :57
            t0 = (tree.lo[inner][None, :, :] - self.o[:, None, :]) * inv[:, None, :]          # :58
            t1 = (tree.hi[inner][None, :, :] - self.o[:, None, :]) * inv[:, None, :]          # :59
            neg = (inv < 0)[:, None, :]                                                       # :60-62
            self.ta, self.tb = np.where(neg, t1, t0).astype(np.float64), np.where(neg, t0, t1).astype(np.float64)
            self.nan = (np.isnan(t0) | np.isnan(t1)).any(axis=2)
            lo, hi = tree.lo[inner][None], tree.hi[inner][None]
            oo = self.o[:, None, :]
            self.inside = ((oo > lo) & (oo < hi)).all(axis=2)
            self.on_face = ((oo >= lo) & (oo <= hi)).all(axis=2) & ((oo == lo) | (oo == hi)).any(axis=2)
            self.t_in = np.fmax.reduce(self.ta, axis=2)                                       # the box alone, without the window
            self.t_out = np.fmin.reduce(self.tb, axis=2)
        n = len(self.o)
        self.G, self.U, self.V, self.UPV, self.T = (np.zeros((tree.A.shape[0], n), np.float32) for _ in range(5))
        for k in range(tree.A.shape[0]):
            A = tree.A[k]
            tt = rb.tri_terms(self.o, self.d, A, A + tree.E1[k], A + tree.E2[k])
            self.G[k], self.U[k], self.V[k], self.UPV[k], self.T[k] = tt["g"], tt["u"], tt["v"], tt["upv"], tt["t"]
        # (a + e1) - a == e1 for lattice corners, so tri_terms sees the stored edges; the host test asserts it
        with np.errstate(**_QUIET):                                                           # :340, :344, :347 with their NaN behaviour
            self.acc = ~(np.abs(self.G) < rb.EPS_G) & ~(self.U < 0) & ~(self.V < 0) & ~(self.UPV > 1)
        self.T64 = self.T.astype(np.float64)

    def trace(self, r, t_max):
        """-> (winner triangle or -1, its distance, events): events maps an interior node below the root to the set of what the walk met
        there: 'nan' (a 0 * inf product), 'edge' (rejected with t_in == t_out, both from box planes, at least two non-zero direction
        components), 'bound' (rejected because its entry distance EQUALS the bound a hit in the left sibling set), 'inside', 'face',
        'ends' (the call's t_max lies strictly between the box's own entry and exit)."""
        tree, tmin0, events = self.tree, float(T_MIN), {}
        nz = int(np.count_nonzero(self.d[r]))
        call_max = float(F(t_max))

        def box(j, bound):
            s = self.slot[j]
            lo_t, hi_t, ok = tmin0, bound, True
            for ax in range(3):
                lo_t, hi_t = _fmax(self.ta[r, s, ax], lo_t), _fmin(self.tb[r, s, ax], hi_t)      # :63-64
                if hi_t <= lo_t:                                                                  # :65
                    ok = False
                    break
            if tree.depth[j] >= 1:
                ev = events.setdefault(j, set())
                if self.nan[r, s]:
                    ev.add("nan")
                if self.inside[r, s]:
                    ev.add("inside")
                if self.on_face[r, s]:
                    ev.add("face")
                ti, to = self.t_in[r, s], self.t_out[r, s]
                if ti < call_max < to and to > tmin0:
                    ev.add("ends")
                if not ok and hi_t == lo_t:
                    if hi_t == bound and bound < call_max and lo_t > tmin0:
                        ev.add("bound")
                    elif ti == to and nz >= 2 and lo_t == ti and hi_t == to:
                        ev.add("edge")
            return ok

        def node(j, bound):
            k = tree.tri[j]
            if k >= 0:                                                                            # :95-97
                t = self.T64[k, r]
                return (t, int(k)) if self.acc[k, r] and not t < tmin0 and not t > bound else None      # :349
            best, best_t = None, bound                                                            # :101-102
            if box(j, bound):                                                                     # :103
                h = node(j + 1, bound)                                                            # :106
                if h is not None:
                    best, best_t = h, h[0]
                h = node(int(tree.end[j + 1]), best_t)                                            # :113
                if h is not None:
                    best = h
            return best

        h = node(0, call_max)
        return (h[1], h[0], events) if h is not None else (-1, 0.0, events)

    def hit_flags(self, r, k, t):
        """What the winning hit (triangle k at distance t) lies on: 'vertex', 'shared edge' (another, non-coincident triangle accepts the same
        distance), 'coincident' (triangle 0 and its copy both accept it)."""
        out = set()
        u, v, upv = self.U[k, r], self.V[k, r], self.UPV[k, r]
        if (u, v) in ((0, 0), (1, 0), (0, 1)):
            out.add("vertex")
        same = np.flatnonzero(self.acc[:, r] & (self.T64[:, r] == t))
        last = self.tree.A.shape[0] - 1
        if (u == 0 or v == 0 or upv == 1) and any(int(x) != k and {int(x), k} != {0, last} for x in same):
            out.add("shared edge")
        if 0 in same and last in same:
            out.add("coincident")
        return out


# ---------------------------------------------------------------------------------------------- candidates, in object space
AXES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
EDGE_DIRS = [(1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 0, -1), (1, 2, -1), (-1, 2, 1), (2, 1, 1), (1, -1, 2), (-2, -1, 1), (0.5, 1, -1)]
GENERIC_DIRS = [(1, 2, -1), (-1, 0.5, 0.25), (0.5, -1, 1), (-0.25, -1, -0.5)]
OUTSIDE = 3.75


def chosen_nodes(tree):
    """Up to three interior nodes below the root per depth whose boxes have extent on every axis, left, right and middle of the level."""
    out = []
    for dep in range(1, int(tree.depth.max()) + 1):
        level = [j for j in tree.inner if tree.depth[j] == dep and (tree.hi[j] > tree.lo[j]).all()]
        out += [level[i] for i in sorted({0, len(level) // 2, len(level) - 1})] if level else []
    return out


def candidates(tree):
    """{kind: [(o, d), ...]} — far more than the table keeps; the walk decides which of them meet their kind."""
    rng = np.random.default_rng(3)
    T = lattice_triangles()
    C = {k: [] for k in ("a", "b", "c", "e", "f")}
    for j in chosen_nodes(tree):
        lo, hi = tree.lo[j].astype(np.float64), tree.hi[j].astype(np.float64)
        mid = 0.5 * (lo + hi)
        for ax in AXES:                                            # a: in a face plane, along axis k
            k = int(np.flatnonzero(ax)[0])
            for m in range(3):
                if m == k:
                    continue
                for plane in (lo[m], hi[m]):
                    o = mid.copy()
                    o[m], o[k] = plane, -OUTSIDE * ax[k]
                    C["a"].append((tuple(o), ax))
        for dr in EDGE_DIRS:                                       # b: through the point whose first non-zero axis sits on its entry plane, the others on exit planes
            dr = np.array(dr, np.float64)
            nzs = [a for a in range(3) if dr[a] != 0]
            for first in (nzs[0], nzs[-1]):
                p = mid.copy()
                for a in nzs:
                    entry, exit_ = (lo[a], hi[a]) if dr[a] > 0 else (hi[a], lo[a])
                    p[a] = entry if a == first else exit_
                C["b"].append((tuple(p - 2.0 * dr), tuple(dr)))
        for dr in AXES + GENERIC_DIRS:                             # f: from the middle of the box, and from the middle of each face
            C["f"].append((tuple(mid), dr))
        for m in range(3):
            for plane in (lo[m], hi[m]):
                o = mid.copy()
                o[m] = plane
                for dr in (AXES[2 * m], AXES[2 * m + 1], GENERIC_DIRS[m]):
                    C["f"].append((tuple(o), dr))
    # c and e: axis-parallel rays at the lattice points, the edge midpoints and the cell centres of both sheets, from above and from below,
    # and along x and z at every lattice height
    for x0, n in ((-3.0, 12), (-1.5, 6)):
        for j in range(2 * n + 1):
            for i in range(2 * n + 1):
                x, z = x0 + 0.25 * i, x0 + 0.25 * j
                C["c"].append(((x, 3.5, z), (0, -1, 0)))
                C["c"].append(((x, -3.5, z), (0, 1, 0)))
    for h in [v / 8.0 for v in list(range(-8, -1)) + list(range(8, 13))]:
        for i in range(13):
            w = -3.0 + 0.5 * i
            C["c"] += [((-OUTSIDE, h, w), (1, 0, 0)), ((OUTSIDE, h, w), (-1, 0, 0)), ((w, h, -OUTSIDE), (0, 0, 1)), ((w, h, OUTSIDE), (0, 0, -1))]
    C["e"] = list(C["c"][:4 * 625:3])
    a, b, c = T[0]
    for wa, wb in ((0.25, 0.25), (0.5, 0.25), (0.25, 0.5), (0.125, 0.125), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5), (0.0, 0.0), (0.625, 0.25), (0.25, 0.125)):
        p = a + wa * (b - a) + wb * (c - a)                        # into the coincident pair: dyadic barycentrics
        for dr in ((0, -1, 0), (0, 1, 0), (0.5, -1, 0.25), (-0.25, 1, 0.5)):
            dr = np.array(dr, np.float64)
            C["e"].append((tuple(p - 2.0 * dr), tuple(dr)))
    generic = []
    for _ in range(64):                                            # no zero component; from above the sheets towards a point of the lower one
        o = np.round(rng.uniform((-3.5, 2.0, -3.5), (3.5, 3.5, 3.5)) * 16) / 16
        to = np.round(rng.uniform((-2.9, -1.0, -2.9), (2.9, -0.25, 2.9)) * 16) / 16 + 1.0 / 32
        generic.append((tuple(o), tuple(to - o)))
    away = [((x, 3.0, z), dr) for (x, z), dr in zip(((0, 0), (1, -1), (-2, 0.5), (2.5, 2.5), (-0.5, -2), (0.25, 1), (3, -3), (-3, 3)),
                                                   ((0.25, 1, 0.125), (0, 1, 0), (-0.5, 1, 0.25), (1, 2, 1), (0, 1, 0.5), (-1, 1, -1), (0.125, 1, 0), (1, 0.5, -1)))]
    return C, generic, away


# ---------------------------------------------------------------------------------------------- the battery
KEEP = 14            # rays kept per kind and flavour (the census asks for 8)


def _arr(pairs):
    return rb.f32([p[0] for p in pairs]).reshape(-1, 3), rb.f32([p[1] for p in pairs]).reshape(-1, 3)


def _spread(idx, n):
    idx = list(idx)
    return idx if len(idx) <= n else [idx[int(i * len(idx) / n)] for i in range(n)]


def battery(tree):
    """-> dict: `o`, `d` the table in OBJECT space ([H * 67, 3] each, entry y * 67 + x; -0.0 where the a- rays have it), `height`, `unique`
    (table index of the first copy of every distinct ray, in rows 32 and up), `kinds` {letter: table indices}, `winner` (triangle per
    entry, -1 = none, main call), `distance`, `calls` (the max_trace_dist values: the main call first), `census`, and `small` — the two
    tables of kind i."""
    C, generic, away = candidates(tree)
    picked = {}
    for kind, want in (("a", "nan"), ("b", "edge"), ("c", "bound"), ("f", None), ("e", None)):
        o, d = _arr(C[kind])
        w = Walk(tree, o, d)
        res = [w.trace(r, FAR) for r in range(len(o))]
        if kind == "a":                                            # per axis and sign, over as many different nodes as possible
            by = {}
            for r, (_, _, ev) in enumerate(res):
                if any("nan" in s for s in ev.values()):
                    by.setdefault(tuple(d[r]), []).append(r)
            picked["a"] = [C["a"][r] for rs in by.values() for r in _spread(rs, 4)]
        elif kind == "f":
            ins = [r for r, (_, _, ev) in enumerate(res) if any("inside" in s for s in ev.values())]
            fac = [r for r, (_, _, ev) in enumerate(res) if any("face" in s for s in ev.values()) and not any("inside" in s for s in ev.values())]
            picked["f"] = [C["f"][r] for r in _spread(ins, KEEP) + _spread(fac, KEEP)]
        elif kind == "e":
            got = {"vertex": [], "shared edge": [], "coincident": []}
            for r, (k, t, _) in enumerate(res):
                if k >= 0:
                    for fl in w.hit_flags(r, k, t):
                        got[fl].append(r)
            picked["e"] = [C["e"][r] for r in sorted(set(_spread(got["vertex"], KEEP) + _spread(got["shared edge"], KEEP) + _spread(got["coincident"], KEEP)))]
        else:
            rs = [r for r, (_, _, ev) in enumerate(res) if any(want in s for s in ev.values())]
            picked[kind] = [C[kind][r] for r in _spread(rs, KEEP + 6)]
    neg_zero = [(o, tuple(-0.0 if c == 0 else c for c in dr)) for o, dr in picked["a"]]
    scaled = [(o, tuple(float(np.ldexp(c, k)) for c in dr)) for k in (20, -20) for kind in ("a", "b", "e", "f") for o, dr in picked[kind]]
    uniq, seen = [], set()
    for p in picked["a"] + neg_zero + picked["b"] + picked["c"] + picked["e"] + picked["f"] + scaled + generic:
        key = (rb.f32(p[0]).tobytes(), rb.f32(p[1]).tobytes())
        if key not in seen:
            seen.add(key)
            uniq.append(p)
    uo, ud = _arr(uniq)
    has_zero = (ud == 0).any(axis=1)
    small_d = np.abs(ud).max(axis=1)
    plain = (small_d > 2.0 ** -10) & (small_d < 2.0 ** 10)
    Z = [p for p, z, ok in zip(uniq, has_zero, plain) if z and ok]
    G = [p for p, z, ok in zip(uniq, has_zero, plain) if not z and ok]
    rows8 = 8 * WIDTH
    table = [Z[i % len(Z)] for i in range(rows8)]
    table += [G[i % len(G)] for i in range(rows8)]
    table += [(Z if i % 2 == 0 else G)[(i // 2) % (len(Z) if i % 2 == 0 else len(G))] for i in range(rows8)]
    both = Z + G
    table += [both[(i // 17) % len(both)] if i % 17 == 0 else away[i % len(away)] for i in range(rows8)]
    first_unique = len(table)
    table += uniq
    while len(table) % WIDTH:
        table.append(table[0])                                     # idle entries repeat ray 0
    o, d = _arr(table)
    height = len(table) // WIDTH
    # ---- the census: the walk over every entry with +0.0 for -0.0 (what object space sees differs per scene and decides nothing: kind a-)
    w = Walk(tree, o, d + F(0.0))
    res = [w.trace(r, FAR) for r in range(len(o))]
    winner = np.array([k for k, _, _ in res], np.int64)
    distance = np.array([t for _, t, _ in res], np.float32)
    uidx = np.arange(first_unique, first_unique + len(uniq))
    ev_any = lambda r, name: any(name in s for s in res[r][2].values())        # noqa: E731
    flags = {r: (w.hit_flags(r, int(winner[r]), float(distance[r])) if winner[r] >= 0 else set()) for r in uidx}
    scale = np.abs(d).max(axis=1)
    unscaled = (scale > 2.0 ** -10) & (scale < 2.0 ** 10)
    kinds = {
        "a": [r for r in uidx if ev_any(r, "nan") and not np.signbit(d[r][d[r] == 0]).any() and unscaled[r]],
        "a-": [r for r in uidx if ev_any(r, "nan") and np.signbit(d[r][d[r] == 0]).any()],
        "b": [r for r in uidx if ev_any(r, "edge") and unscaled[r]],
        "c": [r for r in uidx if ev_any(r, "bound") and unscaled[r]],
        "e vertex": [r for r in uidx if "vertex" in flags[r] and unscaled[r]],
        "e shared edge": [r for r in uidx if "shared edge" in flags[r] and unscaled[r]],
        "e coincident": [r for r in uidx if "coincident" in flags[r] and unscaled[r]],
        "f inside": [r for r in uidx if ev_any(r, "inside") and unscaled[r]],
        "f on a face": [r for r in uidx if ev_any(r, "face") and unscaled[r]],
        "g 2^-20": [r for r in uidx if scale[r] <= 2.0 ** -17 and (ev_any(r, "nan") or ev_any(r, "edge") or ev_any(r, "inside") or ev_any(r, "face") or flags[r])],
        "g 2^20": [r for r in uidx if scale[r] >= 2.0 ** 18],
    }
    # ---- d: three further calls around the distance most unique rays hit at, bit for bit
    hit = uidx[(winner[uidx] >= 0) & unscaled[uidx]]
    vals, counts = np.unique(distance[hit], return_counts=True)
    t_star = F(vals[np.argmax(counts)])
    calls = [FAR, float(t_star), float(np.nextafter(t_star, F(0))), float(np.nextafter(t_star, F(np.inf)))]
    per_call = []
    for tm in calls[1:]:
        rs = [w.trace(r, tm) for r in uidx]
        per_call.append({"hit": int(sum(k >= 0 for k, _, _ in rs)), "at": [int(r) for r, (k, t, _) in zip(uidx, rs) if k >= 0 and F(t) == t_star],
                         "ends": [int(r) for r, (_, _, ev) in zip(uidx, rs) if any("ends" in s for s in ev.values())]})
    at = [int(r) for r in hit if distance[r] == t_star]
    kinds["d hit exactly at max_trace_dist"] = per_call[0]["at"]
    kinds["d max_trace_dist ends inside an interior box"] = per_call[0]["ends"]
    # ---- h: the four stretches, in table entries
    zero_c = (d == 0).any(axis=1)
    enters = np.array([len(res[r][2]) > 0 or winner[r] >= 0 for r in range(len(o))])      # walked past the root
    stretch = lambda k: slice(k * rows8, (k + 1) * rows8)                                  # noqa: E731
    census = {k: len(v) for k, v in kinds.items()}
    census.update({
        "rays": len(o), "unique rays": len(uniq), "height": height, "t*": float(t_star),
        "d hits at t* in the main call": len(at), "d of them lost at max_trace_dist = t* (a box entered exactly there, :65)": len(at) - len(per_call[0]["at"]),
        "d unique rays that hit with max_trace_dist = t*": per_call[0]["hit"], "d one ulp below": per_call[1]["hit"], "d one ulp above": per_call[2]["hit"],
        "d hits at t* one ulp below": len(per_call[1]["at"]), "d hits at t* one ulp above": len(per_call[2]["at"]),
        "h zero-component stretch": int(zero_c[stretch(0)].sum()), "h generic stretch": int((~zero_c[stretch(1)]).sum()),
        "h alternating stretch": int((zero_c[stretch(2)][0::2]).sum() + (~zero_c[stretch(2)][1::2]).sum()),
        "h every 17th enters": int(enters[stretch(3)].sum()), "h entries of that stretch that enter no root": int((~enters[stretch(3)]).sum()),
        "interior nodes below the root that some ray tests": len({j for r in uidx for j in res[r][2]}),
        "depths of the chosen nodes": sorted({int(tree.depth[j]) for j in chosen_nodes(tree)}),
    })
    # ---- i: one entering entry among `away` rays, and none
    lone = [away[i % len(away)] for i in range(WIDTH)]
    none = list(lone)
    lone[41] = Z[0]
    small = {"one enters": _arr(lone), "none enters": _arr(none)}
    return dict(o=o, d=d, height=height, unique=uidx, kinds=kinds, winner=winner, distance=distance, calls=calls, census=census, small=small,
                enters=enters, walk=w)


REQUIRED = ("a", "a-", "b", "c", "d hit exactly at max_trace_dist", "d max_trace_dist ends inside an interior box", "e vertex", "e shared edge",
            "e coincident", "f inside", "f on a face", "g 2^-20", "g 2^20")
