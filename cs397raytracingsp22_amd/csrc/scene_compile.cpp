// scene_compile.cpp — flattens the POD description of the reference's Scene.objects into the device layout of pt_device.h,
// including the BVH of every StaticMesh with the REFERENCE's topology (geometry.rs:190-217: median split of the triangle index
// range, leaf i = triangle i, exact union boxes), emitted in DFS pre-order with skip links for the stackless traversal of
// pt_kernels.hip.  The values hoisted out of the per-ray code (e1, e2, r*r, normalize(e1 x e2), -1/density, albedo/PI, the
// triangle tangent) are computed with the same f32 operations, in the same order, the reference performs per ray.
//
// One stage per part of the scene, run in this order by compile_scene; every check of the descriptor sits in the stage that
// reads that part, so the first error reported is always the same for the same descriptor.
#include "scene_compile.hpp"

#include <algorithm>
#include <cstring>
#include <utility>

#include "bvh_build.hpp"

#pragma clang fp contract(off)

namespace pt {
namespace {

bool finite16(const float* m) { for (int i = 0; i < 16; i++) if (!std::isfinite(m[i])) return false; return true; }

// what the stages hand on to each other
struct Build {
    std::vector<DObject> objs;
    std::vector<DMaterial> mats;
    std::vector<DMesh> meshes;               // per mi_mesh
    std::vector<DMeshF> meshf;
    struct MeshBuild { std::vector<float> nodes, ftris; std::vector<uint32_t> fq; bool qualifies = false, default_ts = false; int inode_end = 0; };
    std::vector<MeshBuild> mb;
    std::vector<int> tex_comb;               // per mi_mesh: its combined maps in `texs`, -1 = none
    std::vector<float> nodes, tris, ftris, e2s, inodes, lnodes;
    std::vector<uint32_t> fnodes;            // the F-trees as the device walks them: 4 words per node (bvh_build.hpp fq_encode)
    std::vector<DTriAttr> attrs;
    std::vector<DTexture> texs;
    std::vector<uint8_t> texels;
    std::vector<DObject> bobjs;              // boundary records of the ConvexVolumes that are not plain spheres
    std::vector<std::pair<size_t, int>> bmesh_fix;   // (record in bobjs, mi_mesh index) to be pointed at its mesh table entry
    std::vector<DMesh> live;                 // the device's mesh table
    std::vector<DMeshF> livef;
    size_t n_scene_meshes = 0;
    std::vector<DObject> list;
    int n_list[4] = { 0, 0, 0, 0 };
    int n_list_lin = 0, top_meshf = -1;
    std::vector<float> obj_rot;
};

int materials(const mi_scene_desc* d, Build& b) {
    const float PI = 3.14159265358979323846f;
    b.mats.resize((size_t)d->n_materials);
    for (int i = 0; i < d->n_materials; i++) {
        const mi_material& s = d->materials[i];
        if (s.kind < MI_MAT_LAMBERTIAN || s.kind > MI_MAT_ISOTROPIC) return fail(MI_ERR_INVALID, "material %d: bad kind %d", i, s.kind);
        DMaterial& m = b.mats[(size_t)i];
        memset(&m, 0, sizeof m);
        m.kind = s.kind;
        for (int k = 0; k < 3; k++) { m.albedo[k] = s.albedo[k]; m.emission[k] = s.emission[k]; m.albedo_over_pi[k] = s.albedo[k] / PI; }
        if (s.kind == MI_MAT_DIELECTRIC) for (int k = 0; k < 3; k++) m.emission[k] = 0.0f;      // materials.rs:102
        m.roughness = s.roughness; m.metallic = s.metallic; m.ior = s.idx_of_refraction;
    }
    return MI_OK;
}

// Texels are padded to RGBA8 on the device: one aligned 4-byte load per fetch instead of three byte loads.  Behind the textures:
// the interleaved copy of a mesh's maps (pt_device.h DMesh.tex_comb) when every bound map has the same size.  A mesh whose texture
// indices are out of range gets none; the mesh stage reports it.
int textures(const mi_scene_desc* d, Build& b) {
    b.texs.resize((size_t)d->n_textures);
    for (int i = 0; i < d->n_textures; i++) {
        const mi_texture& t = d->textures[i];
        if (t.width <= 0 || t.height <= 0 || !t.rgb) return fail(MI_ERR_INVALID, "texture %d: bad size or NULL texels", i);
        while (b.texels.size() % 16) b.texels.push_back(0);
        b.texs[(size_t)i].offset = (uint32_t)b.texels.size();
        b.texs[(size_t)i].width = t.width; b.texs[(size_t)i].height = t.height; b.texs[(size_t)i].pad = 0;
        const size_t np = (size_t)t.width * t.height, at = b.texels.size();
        b.texels.resize(at + np * 4);
        for (size_t k = 0; k < np; k++) {
            b.texels[at + 4 * k] = t.rgb[3 * k]; b.texels[at + 4 * k + 1] = t.rgb[3 * k + 1]; b.texels[at + 4 * k + 2] = t.rgb[3 * k + 2];
            b.texels[at + 4 * k + 3] = 255;
        }
    }
    b.tex_comb.assign((size_t)d->n_meshes, -1);
    for (int mi = 0; mi < d->n_meshes; mi++) {
        const mi_mesh& s = d->meshes[mi];
        if (s.material >= 0) continue;
        int w = 0, h = 0, bound = 0; bool same = true;
        for (int k = 0; k < 5; k++) if (s.textures[k] >= d->n_textures) same = false;
        for (int k = 0; k < 5 && same; k++) if (s.textures[k] >= 0) {
            const mi_texture& t = d->textures[s.textures[k]];
            if (bound == 0) { w = t.width; h = t.height; } else if (t.width != w || t.height != h) same = false;
            bound++;
        }
        if (!(bound >= 2 && same && (uint64_t)w * (uint64_t)h * 16u < (1ull << 30))) continue;
        while (b.texels.size() % 16) b.texels.push_back(0);
        DTexture T; T.offset = (uint32_t)b.texels.size(); T.width = w; T.height = h; T.pad = 0;
        const size_t np = (size_t)w * h, at = b.texels.size();
        b.texels.resize(at + np * 16, 0);
        const uint8_t* src[5];
        for (int k = 0; k < 5; k++) src[k] = s.textures[k] >= 0 ? d->textures[s.textures[k]].rgb : nullptr;
        for (size_t px = 0; px < np; px++) {
            uint8_t* o = &b.texels[at + px * 16];
            // absent maps: albedo 0, emission 0, metallic 0, roughness 1.0 = 255 / 255 (geometry.rs:260-263)
            for (int ch = 0; ch < 3; ch++) { o[ch] = src[0] ? src[0][px * 3 + ch] : 0; o[4 + ch] = src[1] ? src[1][px * 3 + ch] : 0; o[8 + ch] = src[4] ? src[4][px * 3 + ch] : 0; }
            o[3] = src[2] ? src[2][px * 3] : 0;
            o[7] = src[3] ? src[3][px * 3] : 255;
        }
        b.tex_comb[(size_t)mi] = (int)b.texs.size();
        b.texs.push_back(T);
    }
    return MI_OK;
}

// one mesh: its record, de-indexed triangles and attributes, the reference's tree (mesh-local node indices, relocated when it is
// placed) and the F-tree of the two-stage traversal
int mesh(const mi_scene_desc* d, int mi, Build& b) {
    const mi_mesh& s = d->meshes[mi];
    if (!s.positions || !s.normals || !s.texcoords || !s.indices || s.n_triangles < 1 || s.n_vertices < 1)
        return fail(MI_ERR_INVALID, "mesh %d: positions, normals, texcoords and indices are all required (geometry.rs:350,355)", mi);
    for (size_t k = 0; k < 3 * (size_t)s.n_triangles; k++)
        if (s.indices[k] >= (uint32_t)s.n_vertices) return fail(MI_ERR_INVALID, "mesh %d: index %u out of range", mi, s.indices[k]);
    if (!finite16(s.transform) || !finite16(s.inv_transform)) return fail(MI_ERR_INVALID, "mesh %d: non-finite transform", mi);
    if (s.material >= d->n_materials) return fail(MI_ERR_INVALID, "mesh %d: bad material", mi);
    DMesh& M = b.meshes[(size_t)mi];
    memset(&M, 0, sizeof M);
    memcpy(M.transform, s.transform, sizeof M.transform);
    memcpy(M.inv_transform, s.inv_transform, sizeof M.inv_transform);
    M.material = s.material < 0 ? -1 : s.material;
    for (int k = 0; k < 5; k++) {
        if (s.textures[k] >= d->n_textures) return fail(MI_ERR_INVALID, "mesh %d: bad texture index", mi);
        M.tex[k] = s.textures[k] < 0 ? -1 : s.textures[k];
    }
    M.object_index = -1;
    M.tex_comb = b.tex_comb[(size_t)mi];
    M.tri_begin = (int)(b.tris.size() / 12);
    M.n_tris = s.n_triangles;
    Build::MeshBuild& B = b.mb[(size_t)mi];
    build::RefTree rt{ s.positions, s.indices, &B.nodes };
    rt.build(0, s.n_triangles);                                      // geometry.rs:185
    for (int t = 0; t < s.n_triangles; t++) {
        uint32_t ia = s.indices[3 * (size_t)t], ib = s.indices[3 * (size_t)t + 1], ic = s.indices[3 * (size_t)t + 2];
        h3 a = H3p(&s.positions[3 * (size_t)ia]), bb = H3p(&s.positions[3 * (size_t)ib]), cc = H3p(&s.positions[3 * (size_t)ic]);
        h3 e1 = sub(bb, a), e2 = sub(cc, a);                         // geometry.rs:336-337
        float rec[12] = { a.x, a.y, a.z, 0.0f, e1.x, e1.y, e1.z, 0.0f, e2.x, e2.y, e2.z, 0.0f };
        b.tris.insert(b.tris.end(), rec, rec + 12);
        DTriAttr A; memset(&A, 0, sizeof A);
        memcpy(A.na, &s.normals[3 * (size_t)ia], 12); memcpy(A.nb, &s.normals[3 * (size_t)ib], 12); memcpy(A.nc, &s.normals[3 * (size_t)ic], 12);
        memcpy(A.ta, &s.texcoords[2 * (size_t)ia], 8); memcpy(A.tb, &s.texcoords[2 * (size_t)ib], 8); memcpy(A.tc, &s.texcoords[2 * (size_t)ic], 8);
        // StaticMesh::get_tangent geometry.rs:245-250
        float u1 = A.ta[0], u2 = A.tb[0], u3 = A.tc[0], v1 = A.ta[1], v2 = A.tb[1], v3 = A.tc[1];
        h3 num = sub(scale(sub(bb, a), (v3 - v1)), scale(sub(cc, a), (v2 - v1)));
        float den = (u2 - u1) * (v3 - v1) - (v2 - v1) * (u3 - u1);
        A.tan[0] = num.x / den; A.tan[1] = num.y / den; A.tan[2] = num.z / den;
        b.attrs.push_back(A);
    }
    // Two-stage traversal (bvh_build.hpp): does the padding bound apply to this mesh?  B = 7 eps E2 |d_obj| / 1e-4 must
    // stay <= 1/2 for every ray; |d_obj| <= |inv_transform's 3x3|_F |d_world|, and world directions of up to 8 units are
    // covered with a factor 10 to spare (a longer one takes the reference walk for that ray, decided on the device).
    DMeshF& F = b.meshf[(size_t)mi];
    memset(&F, 0, sizeof F);
    std::vector<float> fnodes;
    build::FTree ft{ b.tris.data() + (size_t)M.tri_begin * 12, s.n_triangles, &fnodes, &B.ftris, 0, 2, {}, {}, {} };
    const build::FConst fc = ft.run();
    double fro = 0.0;
    for (int cc = 0; cc < 3; cc++) for (int r = 0; r < 3; r++) fro += (double)s.inv_transform[cc * 4 + r] * (double)s.inv_transform[cc * 4 + r];
    const double b_ref = 7.0 * 5.9604645e-08 * (double)fc.E2 * (std::sqrt(fro) * 8.0) * 1.0e4;
    const bool affine = s.inv_transform[3] == 0.0f && s.inv_transform[7] == 0.0f && s.inv_transform[11] == 0.0f && s.inv_transform[15] == 1.0f;
    B.qualifies = affine && std::isfinite(b_ref) && b_ref <= 0.05 && s.n_triangles < (1 << 24) && std::isfinite(fc.R) && std::isfinite(fc.L);
    build::FQuant fq{ 1.0f, 0.0f, 0.0f, 0.0f };
    if (B.qualifies) B.qualifies = build::fq_encode(fnodes.data(), fnodes.size() / 8, &fq, &B.fq);
    F.qs = fq.s; F.qbx = fq.bx; F.qby = fq.by; F.qbz = fq.bz;
    B.default_ts = B.qualifies && s.n_triangles >= 1024;        // below that the reference's tree sits in LDS and the F-tree does not pay
    F.qualifies = B.qualifies ? 1 : 0;
    F.E2 = fc.E2; F.L = fc.L; F.cx = fc.cx; F.cy = fc.cy; F.cz = fc.cz; F.R = fc.R;
    if (!B.qualifies) { B.fq.clear(); B.ftris.clear(); }
    return MI_OK;
}

// one mesh's trees into the pools: the reference's tree (node pool; e2 pool), the same tree as interior and leaf records with explicit
// links (pt_device.h DScene.inodes), and its F-tree
void place_mesh(int mi, Build& b) {
    Build::MeshBuild& B = b.mb[(size_t)mi];
    DMesh& M = b.meshes[(size_t)mi];
    DMeshF& F = b.meshf[(size_t)mi];
    const int nbase = (int)(b.nodes.size() / 8), fbase = (int)(b.fnodes.size() / 4);
    M.node_begin = nbase;
    for (size_t k = 0; k < B.nodes.size(); k += 8) { int sk; memcpy(&sk, &B.nodes[k + 3], 4); sk += nbase; memcpy(&B.nodes[k + 3], &sk, 4); }
    // leaf nodes carry {a, skip}{e1, tri} instead of their (never tested) box; e2 goes to its own small pool
    M.e2_begin = (int)(b.e2s.size() / 4);
    for (size_t k = 0; k < B.nodes.size(); k += 8) {
        int tri; memcpy(&tri, &B.nodes[k + 7], 4);
        if (tri < 0) continue;
        const float* T = &b.tris[((size_t)M.tri_begin + (size_t)tri) * 12];
        B.nodes[k + 0] = T[0]; B.nodes[k + 1] = T[1]; B.nodes[k + 2] = T[2];
        B.nodes[k + 4] = T[4]; B.nodes[k + 5] = T[5]; B.nodes[k + 6] = T[6];
    }
    for (int t = 0; t < M.n_tris; t++) {
        const float* T = &b.tris[((size_t)M.tri_begin + (size_t)t) * 12];
        const float rec[4] = { T[8], T[9], T[10], 0.0f };
        b.e2s.insert(b.e2s.end(), rec, rec + 4);
    }
    const int n_local = (int)(B.nodes.size() / 8);
    const int ibase = (int)(b.inodes.size() / 8), lbase = (int)(b.lnodes.size() / 12);
    std::vector<int32_t> id((size_t)n_local);
    int ni = 0, nl = 0;
    for (int j = 0; j < n_local; j++) {
        int tri; memcpy(&tri, &B.nodes[(size_t)j * 8 + 7], 4);
        id[(size_t)j] = tri < 0 ? ibase + ni++ : ~(lbase + nl++);
    }
    auto id_of = [&](int j) -> int32_t { return j >= n_local ? kIdEnd : id[(size_t)j]; };
    for (int j = 0; j < n_local; j++) {
        const float* N = &B.nodes[(size_t)j * 8];
        int sk, tri; memcpy(&sk, &N[3], 4); memcpy(&tri, &N[7], 4);
        if (tri < 0) {
            float rec[8] = { N[0], N[1], N[2], 0.0f, N[4], N[5], N[6], 0.0f };
            const int32_t miss = id_of(sk - nbase), hit = id_of(j + 1);
            memcpy(&rec[3], &miss, 4); memcpy(&rec[7], &hit, 4);
            b.inodes.insert(b.inodes.end(), rec, rec + 8);
        } else {
            const float* T = &b.tris[((size_t)M.tri_begin + (size_t)tri) * 12];
            float rec[12] = { T[0], T[1], T[2], 0.0f, T[4], T[5], T[6], 0.0f, T[8], T[9], T[10], 0.0f };
            const int32_t next = id_of(j + 1);
            memcpy(&rec[3], &next, 4); memcpy(&rec[7], &tri, 4);
            b.lnodes.insert(b.lnodes.end(), rec, rec + 12);
        }
    }
    M.i_root = id_of(0);
    B.inode_end = (int)(b.inodes.size() / 8);
    b.nodes.insert(b.nodes.end(), B.nodes.begin(), B.nodes.end());
    M.node_end = (int)(b.nodes.size() / 8);
    for (size_t k = 0; k < B.fq.size(); k += 4) if (!(B.fq[k + 3] & 0x80000000u)) B.fq[k + 3] += (uint32_t)fbase;      // interior nodes: skip links into the pool
    F.fnode_begin = fbase; F.ftri_begin = (int)(b.ftris.size() / 12);
    b.fnodes.insert(b.fnodes.end(), B.fq.begin(), B.fq.end());
    b.ftris.insert(b.ftris.end(), B.ftris.begin(), B.ftris.end());
    F.fnode_end = (int)(b.fnodes.size() / 4);
    B.nodes.clear(); B.nodes.shrink_to_fit(); B.fq.clear(); B.ftris.clear();
}

// Pool placement: meshes walked through the reference's tree first, so that one LDS window over the head of the node
// pool covers exactly the trees wf_trav needs.  (The order of Scene.objects — ties, RNG draws — is not touched.)
// Who references which mesh: Scene.objects entries, and ConvexVolume boundaries (a StaticMesh, or a nested Scene's entries).
// Trees nobody references are not placed at all; boundary-only trees go last (they are walked from global memory).
int place_meshes(const mi_scene_desc* d, Build& b) {
    std::vector<uint8_t> obj_ref((size_t)d->n_meshes, 0), bnd_ref((size_t)d->n_meshes, 0);
    if (d->n_boundary_objects < 0 || (d->n_boundary_objects > 0 && !d->boundary_objects)) return fail(MI_ERR_INVALID, "bad boundary_objects");
    for (int i = 0; i < d->n_objects; i++)
        if (d->objects[i].kind == MI_OBJ_MESH) {
            if (d->objects[i].index < 0 || d->objects[i].index >= d->n_meshes) return fail(MI_ERR_INVALID, "object %d: bad mesh index", i);
            obj_ref[(size_t)d->objects[i].index] = 1;
        }
    for (int v = 0; v < d->n_volumes && d->volumes; v++) {
        const mi_volume& vo = d->volumes[v];
        auto mark = [&](int kind, int index) -> int {
            if (kind == MI_OBJ_MESH) {
                if (index < 0 || index >= d->n_meshes) return fail(MI_ERR_INVALID, "volume %d: bad boundary mesh index", v);
                bnd_ref[(size_t)index] = 1;
            }
            return MI_OK;
        };
        if (vo.boundary_kind == MI_OBJ_SCENE) {
            if (vo.boundary_index < 0 || vo.boundary_count < 0 || (int64_t)vo.boundary_index + vo.boundary_count > d->n_boundary_objects)
                return fail(MI_ERR_INVALID, "volume %d: boundary entries out of range", v);
            for (int k = 0; k < vo.boundary_count; k++) {
                const mi_object& e = d->boundary_objects[vo.boundary_index + k];
                const int rcm = mark(e.kind, e.index);
                if (rcm != MI_OK) return rcm;
            }
        } else {
            const int rcm = mark(vo.boundary_kind, vo.boundary_index);
            if (rcm != MI_OK) return rcm;
        }
    }
    for (int pass = 0; pass < 3; pass++)
        for (int mi = 0; mi < d->n_meshes; mi++) {
            const int cls = obj_ref[(size_t)mi] ? (b.mb[(size_t)mi].default_ts ? 1 : 0) : (bnd_ref[(size_t)mi] ? 2 : 3);
            if (cls == pass) place_mesh(mi, b);
        }
    return MI_OK;
}

// one Sphere / Triangle / Plane record (Scene.objects entry or boundary entry), derived constants hoisted
int primitive(const mi_scene_desc* d, int kind, int index, const char* what, int i, DObject& D) {
    auto mat_ok = [&](int id) { return id >= 0 && id < d->n_materials; };
    switch (kind) {
    case MI_OBJ_SPHERE: {
        if (index < 0 || index >= d->n_spheres || !d->spheres) return fail(MI_ERR_INVALID, "%s %d: bad sphere index", what, i);
        const mi_sphere& s = d->spheres[index];
        if (!mat_ok(s.material)) return fail(MI_ERR_INVALID, "%s %d: bad material", what, i);
        D.material = s.material;
        D.f[0] = s.center[0]; D.f[1] = s.center[1]; D.f[2] = s.center[2]; D.f[3] = s.radius;
        D.f[4] = s.radius * s.radius;                               // geometry.rs:400
        return MI_OK;
    }
    case MI_OBJ_TRIANGLE: {
        if (index < 0 || index >= d->n_triangles || !d->triangles) return fail(MI_ERR_INVALID, "%s %d: bad triangle index", what, i);
        const mi_triangle& t = d->triangles[index];
        if (!mat_ok(t.material)) return fail(MI_ERR_INVALID, "%s %d: bad material", what, i);
        D.material = t.material;
        h3 a = H3p(t.a), e1 = sub(H3p(t.b), a), e2 = sub(H3p(t.c), a);      // geometry.rs:434-435
        h3 n = normalize(cross(e1, e2));                                    // geometry.rs:449
        D.f[0] = a.x; D.f[1] = a.y; D.f[2] = a.z;
        D.f[3] = e1.x; D.f[4] = e1.y; D.f[5] = e1.z;
        D.f[6] = e2.x; D.f[7] = e2.y; D.f[8] = e2.z;
        D.f[9] = n.x; D.f[10] = n.y; D.f[11] = n.z;
        return MI_OK;
    }
    case MI_OBJ_PLANE: {
        if (index < 0 || index >= d->n_planes || !d->planes) return fail(MI_ERR_INVALID, "%s %d: bad plane index", what, i);
        const mi_plane& p = d->planes[index];
        if (!mat_ok(p.material)) return fail(MI_ERR_INVALID, "%s %d: bad material", what, i);
        D.material = p.material;
        for (int k = 0; k < 3; k++) { D.f[k] = p.point[k]; D.f[3 + k] = p.normal[k]; }
        return MI_OK;
    }
    default: return fail(MI_ERR_INVALID, "%s %d: unknown kind %d", what, i, kind);
    }
}

// Scene.objects in order, and the boundary records of the ConvexVolumes that are not plain spheres (boundary meshes get entries of
// the device's mesh table BEHIND the Scene.objects meshes: bmesh_fix, resolved by mesh_table)
int scene_objects(const mi_scene_desc* d, Build& b) {
    b.objs.resize((size_t)d->n_objects);
    for (int i = 0; i < d->n_objects; i++) {
        const mi_object& o = d->objects[i];
        DObject& D = b.objs[(size_t)i];
        memset(&D, 0, sizeof D);
        D.kind = o.kind;
        D.index = i;
        D.ref = -1;
        switch (o.kind) {
        case MI_OBJ_SPHERE: case MI_OBJ_TRIANGLE: case MI_OBJ_PLANE: {
            const int rcp = primitive(d, o.kind, o.index, "object", i, D);
            if (rcp != MI_OK) return rcp;
            break;
        }
        case MI_OBJ_VOLUME: {
            if (o.index < 0 || o.index >= d->n_volumes || !d->volumes) return fail(MI_ERR_INVALID, "object %d: bad volume index", i);
            const mi_volume& v = d->volumes[o.index];
            if (v.phase_material < 0 || v.phase_material >= d->n_materials) return fail(MI_ERR_INVALID, "object %d: bad phase material", i);
            D.material = v.phase_material;
            D.f[5] = -1.0f / v.density;                                 // geometry.rs:517
            if (v.boundary_kind == MI_OBJ_SPHERE) {                     // the inline sphere: what every use in the reference is
                for (int k = 0; k < 3; k++) D.f[k] = v.boundary_center[k];
                D.f[3] = v.boundary_radius;
                D.f[4] = v.boundary_radius * v.boundary_radius;         // geometry.rs:400 via :505
                break;
            }
            // any other `Arc<dyn Intersectable>` (geometry.rs:496): its records, tested twice per ray by the kernels (:505,508)
            std::vector<mi_object> entries;
            if (v.boundary_kind == MI_OBJ_SCENE) for (int k = 0; k < v.boundary_count; k++) entries.push_back(d->boundary_objects[v.boundary_index + k]);
            else { mi_object e; e.kind = v.boundary_kind; e.index = v.boundary_index; entries.push_back(e); }
            D.ref = (int)b.bobjs.size();
            { const int n = (int)entries.size(); memcpy(&D.f[6], &n, 4); }
            for (size_t k = 0; k < entries.size(); k++) {
                DObject R; memset(&R, 0, sizeof R);
                R.kind = entries[k].kind; R.index = (int)k; R.ref = -1;
                if (entries[k].kind == MI_OBJ_MESH) { R.material = -1; b.bmesh_fix.emplace_back(b.bobjs.size(), entries[k].index); }
                else if (entries[k].kind == MI_OBJ_VOLUME || entries[k].kind == MI_OBJ_SCENE)
                    return fail(MI_ERR_UNSUPPORTED, "object %d: a ConvexVolume or a Scene inside a ConvexVolume boundary", i);
                else { const int rcp = primitive(d, entries[k].kind, entries[k].index, "boundary entry of object", i, R); if (rcp != MI_OK) return rcp; }
                b.bobjs.push_back(R);
            }
            break;
        }
        case MI_OBJ_MESH: {
            // the same StaticMesh may appear several times (Arc sharing, tracing.rs:215): every appearance is an entry of its own
            // in the device's mesh table — sharing the nodes, triangles and attributes in the pools — with its own object index
            D.ref = o.index; D.material = -1;
            break;
        }
        default: return fail(MI_ERR_INVALID, "object %d: unknown kind %d", i, o.kind);
        }
    }
    return MI_OK;
}

// The device's mesh table: one entry per MESH entry of Scene.objects, in that order (S.n_meshes of them: what the hit loop
// walks), then one per boundary mesh (reached only through a ConvexVolume's boundary record).
void mesh_table(Build& b, CompiledScene& out) {
    for (DObject& o : b.objs)
        if (o.kind == OBJ_MESH) {
            const int r = o.ref; o.ref = (int)b.live.size();
            b.live.push_back(b.meshes[(size_t)r]); b.livef.push_back(b.meshf[(size_t)r]);
            b.live.back().object_index = o.index;
            const Build::MeshBuild& B = b.mb[(size_t)r];
            CompiledScene::Mesh m{};
            m.node_end = b.meshes[(size_t)r].node_end; m.inode_end = B.inode_end; m.qualifies = B.qualifies; m.default_ts = B.default_ts;
            out.meshes.push_back(m);
        }
    b.n_scene_meshes = b.live.size();
    for (auto& fx : b.bmesh_fix) {
        b.bobjs[fx.first].ref = (int)b.live.size();
        b.live.push_back(b.meshes[(size_t)fx.second]); b.livef.push_back(b.meshf[(size_t)fx.second]);
        b.live.back().object_index = -1;
    }
}

// kind-grouped copy of the non-mesh objects (stable within a kind), and the top-level tree over its Triangles
// ("top-level BVH over Scene.objects"; long lists only).
// A list of hundreds of Triangles is hundreds of Moller-Trumbore tests per path segment.  The exact two-stage machinery of the
// meshes applies to them unchanged, in world space: a SAH tree over the triangles' boxes, walked per ray with the boxes padded by the
// proven bound on what the reference's f32 test can accept (bvh_build.hpp), and the reference's own test on the triangles of the leaves
// reached — a triangle whose padded box the ray misses would have failed that test, and the closest hit over the rest is
// order-independent (ties: the lower Scene.objects index).  The bound scales with E2 = max |e1||e2| over the tree, so the LARGE
// triangles (walls: 32 x the median product and more) stay in front of the list and are tested one by one; the tree needs >= 96 of
// the others.  A ray the bound does not cover (B > 1/2, non-finite) makes its wave test the whole list one by one.
void object_list(Build& b) {
    const int order[4] = { OBJ_TRIANGLE, OBJ_SPHERE, OBJ_PLANE, OBJ_VOLUME };
    for (int g = 0; g < 4; g++)
        for (size_t i = 0; i < b.objs.size(); i++)
            if (b.objs[i].kind == order[g]) { b.list.push_back(b.objs[i]); b.n_list[g]++; }
    b.n_list_lin = b.n_list[0];
    constexpr int kTopMinTris = 96;       // measured (tools/probe_list_tree.py): 40 small triangles 0.85 x, 105: 1.1 x, 400: 1.6 x, 2000: 1.9 x of the plain loop
    const int nt = b.n_list[0];
    if (nt < kTopMinTris) return;
    std::vector<double> prod((size_t)nt);
    for (int k = 0; k < nt; k++) {
        const float* f = b.list[(size_t)k].f;
        prod[(size_t)k] = std::sqrt((double)f[3] * f[3] + (double)f[4] * f[4] + (double)f[5] * f[5]) * std::sqrt((double)f[6] * f[6] + (double)f[7] * f[7] + (double)f[8] * f[8]);
    }
    std::vector<double> sorted = prod;
    std::nth_element(sorted.begin(), sorted.begin() + nt / 2, sorted.end());
    const double big = 32.0 * sorted[(size_t)nt / 2];
    // large triangles (and anything non-finite) to the front, order kept within each part (stable: ties between equal hits are decided by index anyway)
    std::vector<DObject> front, rest;
    for (int k = 0; k < nt; k++) ((!(prod[(size_t)k] <= big) || !std::isfinite(prod[(size_t)k])) ? front : rest).push_back(b.list[(size_t)k]);
    if ((int)rest.size() < kTopMinTris) return;
    std::vector<float> lt(rest.size() * 12, 0.0f), tn, tt;
    for (size_t k = 0; k < rest.size(); k++) {
        const float* f = rest[k].f; float* T = &lt[k * 12];
        for (int q = 0; q < 3; q++) { T[q] = f[q]; T[4 + q] = f[3 + q]; T[8 + q] = f[6 + q]; }
    }
    build::FTree ft{ lt.data(), (int)rest.size(), &tn, &tt, 0, 2, {}, {}, {} };
    const build::FConst fc = ft.run();
    build::FQuant fq{ 1.0f, 0.0f, 0.0f, 0.0f };
    std::vector<uint32_t> tq;
    // (the bound's B = 7 eps E2 |d| / 1e-4 is checked per ray on the device; here only: is it finite, and below 1/2 for a unit direction at all)
    const double b_unit = 7.0 * 5.9604645e-08 * (double)fc.E2 * 1.0e4;
    if (!(std::isfinite(b_unit) && b_unit <= 0.25 && std::isfinite(fc.R) && std::isfinite(fc.L) && rest.size() < (1u << 24) &&
          build::fq_encode(tn.data(), tn.size() / 8, &fq, &tq))) return;
    const int fbase = (int)(b.fnodes.size() / 4);
    for (size_t k = 0; k < tq.size(); k += 4) if (!(tq[k + 3] & 0x80000000u)) tq[k + 3] += (uint32_t)fbase;      // interior nodes: skip links into the pool
    for (size_t e = 0; e < tt.size() / 12; e++) {          // a leaf triangle carries its Scene.objects index where a mesh triangle carries its number
        int t; memcpy(&t, &tt[e * 12 + 3], 4);
        const int32_t idx = rest[(size_t)t].index;
        memcpy(&tt[e * 12 + 3], &idx, 4);
    }
    DMeshF F; memset(&F, 0, sizeof F);
    F.fnode_begin = fbase; F.ftri_begin = (int)(b.ftris.size() / 12);
    b.fnodes.insert(b.fnodes.end(), tq.begin(), tq.end());
    b.ftris.insert(b.ftris.end(), tt.begin(), tt.end());
    F.fnode_end = (int)(b.fnodes.size() / 4);
    F.qualifies = 1; F.E2 = fc.E2; F.L = fc.L; F.cx = fc.cx; F.cy = fc.cy; F.cz = fc.cz; F.R = fc.R;
    F.qs = fq.s; F.qbx = fq.bx; F.qby = fq.by; F.qbz = fq.bz;
    b.top_meshf = (int)b.livef.size();
    b.livef.push_back(F);
    b.n_list_lin = (int)front.size();
    for (size_t k = 0; k < front.size(); k++) b.list[k] = front[k];
    for (size_t k = 0; k < rest.size(); k++) b.list[front.size() + k] = rest[k];
}

// world-space corners of the root boxes (tile masks).  The rays reach object space through inv_transform
// (geometry.rs:304), so the corners come from ITS inverse (f64), not from `transform`; a projective
// inv_transform or a single-triangle mesh (no root box) is never culled.
void root_boxes(const Build& b, CompiledScene& out) {
    for (size_t m = 0; m < b.n_scene_meshes; m++) {
        const DMesh& M = b.live[m];
        const float* it = M.inv_transform;
        if (!(it[3] == 0.0f && it[7] == 0.0f && it[11] == 0.0f && it[15] == 1.0f)) continue;
        const float* n0 = &b.nodes[(size_t)M.node_begin * 8];
        int32_t tri_id; memcpy(&tri_id, &n0[7], 4);
        if (tri_id >= 0) continue;
        double a[4][8];                                   // [inv | I], Gauss-Jordan with partial pivoting
        for (int r = 0; r < 4; r++) for (int q = 0; q < 4; q++) { a[r][q] = (double)it[q * 4 + r]; a[r][4 + q] = r == q ? 1.0 : 0.0; }
        bool ok = true;
        for (int col = 0; col < 4 && ok; col++) {
            int piv = col;
            for (int r = col + 1; r < 4; r++) if (fabs(a[r][col]) > fabs(a[piv][col])) piv = r;
            if (!(fabs(a[piv][col]) > 1e-12)) { ok = false; break; }
            if (piv != col) for (int q = 0; q < 8; q++) std::swap(a[piv][q], a[col][q]);
            const double inv = 1.0 / a[col][col];
            for (int q = 0; q < 8; q++) a[col][q] *= inv;
            for (int r = 0; r < 4; r++) if (r != col) { const double f = a[r][col]; for (int q = 0; q < 8; q++) a[r][q] -= f * a[col][q]; }
        }
        if (!ok) continue;
        CompiledScene::Mesh& B = out.meshes[m];
        B.cullable = true;
        for (int k = 0; k < 8; k++) {
            const double q[3] = { (double)((k & 1) ? n0[4] : n0[0]), (double)((k & 2) ? n0[5] : n0[1]), (double)((k & 4) ? n0[6] : n0[2]) };
            for (int r = 0; r < 3; r++) {
                B.corner[k][r] = a[r][4] * q[0] + a[r][5] * q[1] + a[r][6] * q[2] + a[r][7];
                if (!std::isfinite(B.corner[k][r])) B.cullable = false;
            }
        }
    }
}

// sample_hemisphere's rotation Basis3::between_vectors(unit_y, n) (materials.rs:176) as a matrix, for the two normals a list Triangle or Plane can
// present to a ray (its stored normal and the negation: RayHit::new, tracing.rs:118-123; Plane: geometry.rs:476-478): the same f32 operations in the same order as
// pt_kernels.hip rotate_from_unit_y performs per scatter (this file is compiled with -ffp-contract=off; sqrtf and the divisions are
// correctly rounded on both sides, rcp_exact IS 1.0f / x), so reading the table is exact.  12 floats per entry:
// {c0.xyz, c1.x}{c1.yz, c2.xy}{c2.z, 1 = identity (the function returns `dir` untouched), 0, 0}; entry 2 i + (frontface ? 0 : 1) of object i.
void rotations(Build& b) {
    auto ulps_eq = [](float a, float c) {                       // approx::ulps_eq!, f32 defaults (pt_kernels.hip ulps_eq)
        if (fabsf(a - c) <= 1.1920929e-07f) return true;
        if ((a < 0.0f) != (c < 0.0f)) return false;
        int32_t ia, ic; memcpy(&ia, &a, 4); memcpy(&ic, &c, 4);
        int32_t d = (int32_t)((uint32_t)ia - (uint32_t)ic);
        if (d < 0) d = (int32_t)(0u - (uint32_t)d);
        return d <= 4;
    };
    auto rot = [&](float nx, float ny, float nz, float* out) {
        const float k_cos_theta = ny;
        if (ulps_eq(k_cos_theta, 1.0f)) { out[9] = 1.0f; return; }
        const float k = sqrtf(1.0f * ((nx * nx + ny * ny) + nz * nz));
        float qs, qx, qz;
        if (ulps_eq(k_cos_theta / k, -1.0f)) { qs = 0.0f; qx = 0.0f; qz = -1.0f; }
        else {
            const float sq = k + k_cos_theta;
            const float cx = nz, cz = -nx;
            const float mag = sqrtf(sq * sq + ((cx * cx + 0.0f) + cz * cz));
            const float inv = 1.0f / mag;
            qs = sq * inv; qx = cx * inv; qz = cz * inv;
        }
        const float x2 = qx + qx, z2 = qz + qz;
        const float xx2 = x2 * qx, xz2 = x2 * qz, zz2 = z2 * qz;
        const float sz2 = z2 * qs, sx2 = x2 * qs;
        out[0] = 1.0f - zz2; out[1] = sz2; out[2] = xz2;                       // c0
        out[3] = -sz2; out[4] = (1.0f - xx2) - zz2; out[5] = sx2;            // c1
        out[6] = xz2; out[7] = -sx2; out[8] = 1.0f - xx2;                     // c2
        // A matrix that IS the identity as values (a normal along +y of any length: the early return above takes only n.y within
        // ulps_eq of 1, i.e. f32 epsilon or 4 ulp) is stored as one: the reference multiplies by it, which returns `dir` up to the sign
        // of a zero component (its x * 1 + y * 0 + z * 0 can turn a -0 into +0; the flag keeps -0: DESIGN.md section 2 (vi)).  A NaN (the normal of a zero-area Triangle) is stored as THE quiet NaN:
        // which NaN an operation on NaNs returns — sign, payload — depends on the operand order the compiler chose, and the blob's
        // bytes must not depend on who compiled this file.
        bool ident = true;
        for (int k = 0; k < 9; k++) ident = ident && out[k] == ((k % 4 == 0) ? 1.0f : 0.0f);
        if (ident) { for (int k = 0; k < 9; k++) out[k] = 0.0f; out[9] = 1.0f; return; }
        const uint32_t qnan = 0x7fc00000u;
        for (int k = 0; k < 9; k++) if (out[k] != out[k]) memcpy(&out[k], &qnan, 4);
    };
    b.obj_rot.assign(b.objs.size() * 24, 0.0f);
    for (size_t i = 0; i < b.objs.size(); i++) if (b.objs[i].kind == OBJ_TRIANGLE || b.objs[i].kind == OBJ_PLANE) {
        const float* n = b.objs[i].f + (b.objs[i].kind == OBJ_TRIANGLE ? 9 : 3);       // the Triangle's stored normal / the Plane's
        rot(n[0], n[1], n[2], &b.obj_rot[i * 24]);
        rot(-n[0], -n[1], -n[2], &b.obj_rot[i * 24 + 12]);
    }
}

// the blob's layout and host image, and the scene's counts
int layout(const Build& b, CompiledScene& out) {
    auto align = [](size_t x) { return (x + 255) & ~(size_t)255; };
    CompiledScene::Offsets& o = out.off;
    o.obj = 0;
    o.list = align(o.obj + b.objs.size() * sizeof(DObject));
    o.bobj = align(o.list + (b.list.size() + 1) * sizeof(DObject));     // +1: the loop prefetches one record ahead
    o.rot = align(o.bobj + (b.bobjs.size() + 1) * sizeof(DObject));
    o.mat = align(o.rot + b.obj_rot.size() * 4 + 16);
    o.mesh = align(o.mat + b.mats.size() * sizeof(DMaterial));
    o.meshf = align(o.mesh + b.live.size() * sizeof(DMesh));
    o.fnodes = align(o.meshf + b.livef.size() * sizeof(DMeshF));
    o.ftris = align(o.fnodes + b.fnodes.size() * 4 + 32);
    o.nodes = align(o.ftris + b.ftris.size() * 4 + 48);
    o.e2 = align(o.nodes + b.nodes.size() * 4);
    o.inodes = align(o.e2 + b.e2s.size() * 4 + 16);
    o.lnodes = align(o.inodes + b.inodes.size() * 4 + 32);
    o.tris = align(o.lnodes + b.lnodes.size() * 4 + 48);
    o.attr = align(o.tris + b.tris.size() * 4);
    o.tex = align(o.attr + b.attrs.size() * sizeof(DTriAttr));
    o.texel = align(o.tex + b.texs.size() * sizeof(DTexture));
    const size_t total = align(o.texel + b.texels.size() + 16);
    if (total > 0xffffffffull) return fail(MI_ERR_UNSUPPORTED, "scene larger than 4 GiB");
    out.image.assign(total, 0);
    auto put = [&](size_t off, const void* p, size_t n) { if (n) memcpy(out.image.data() + off, p, n); };
    put(o.obj, b.objs.data(), b.objs.size() * sizeof(DObject));
    put(o.list, b.list.data(), b.list.size() * sizeof(DObject));
    put(o.bobj, b.bobjs.data(), b.bobjs.size() * sizeof(DObject));
    put(o.rot, b.obj_rot.data(), b.obj_rot.size() * 4);
    put(o.mat, b.mats.data(), b.mats.size() * sizeof(DMaterial));
    put(o.mesh, b.live.data(), b.live.size() * sizeof(DMesh));
    put(o.meshf, b.livef.data(), b.livef.size() * sizeof(DMeshF));
    put(o.fnodes, b.fnodes.data(), b.fnodes.size() * 4);
    put(o.ftris, b.ftris.data(), b.ftris.size() * 4);
    put(o.nodes, b.nodes.data(), b.nodes.size() * 4);
    put(o.e2, b.e2s.data(), b.e2s.size() * 4);
    put(o.inodes, b.inodes.data(), b.inodes.size() * 4);
    put(o.lnodes, b.lnodes.data(), b.lnodes.size() * 4);
    put(o.tris, b.tris.data(), b.tris.size() * 4);
    put(o.attr, b.attrs.data(), b.attrs.size() * sizeof(DTriAttr));
    put(o.tex, b.texs.data(), b.texs.size() * sizeof(DTexture));
    put(o.texel, b.texels.data(), b.texels.size());
    DScene& S = out.S;
    S.n_list_tri = b.n_list[0]; S.n_list_sphere = b.n_list[1]; S.n_list_plane = b.n_list[2]; S.n_list_volume = b.n_list[3];
    S.n_list_lin = b.n_list_lin; S.top_meshf = b.top_meshf;
    S.n_fnodes = (int)(b.fnodes.size() / 4);
    S.n_objects = (int)b.objs.size();
    S.n_meshes = (int)b.n_scene_meshes;
    S.n_nodes = (int)(b.nodes.size() / 8);
    S.n_tris = (int)(b.tris.size() / 12);
    return MI_OK;
}

// The may-emit flags (scene_compile.hpp EmitFlags) of Scene.objects, of the kind-grouped list and of the live meshes
EmitFlags emit_flags(const mi_scene_desc* d, const Build& b) {
    EmitFlags e;
    auto mat = [&](int id) { return material_may_emit(d->materials[id]); };
    auto mesh = [&](const DMesh& M) { return (M.material >= 0 && mat(M.material)) || M.tex[1] >= 0; };
    auto object = [&](const DObject& o) { return o.kind == OBJ_MESH ? mesh(b.live[(size_t)o.ref]) : mat(o.material); };
    e.object_bits.assign(b.objs.size() / 32 + 1, 0u);
    for (size_t i = 0; i < b.objs.size(); i++) if (object(b.objs[i])) e.object_bits[i / 32] |= 1u << (i % 32);
    for (const DObject& o : b.list) if (o.kind == OBJ_VOLUME && object(o)) e.any_volume = true;
    e.list_mask_valid = b.list.size() <= 64;
    for (size_t k = 0; k < b.list.size() && k < 64; k++) if (object(b.list[k])) e.list_mask |= 1ull << k;
    for (size_t m = 0; m < b.n_scene_meshes; m++)
        if (mesh(b.live[m])) { e.any_mesh = true; if (m < 32) e.mesh_mask |= 1u << m; }
    return e;
}

}  // namespace

bool material_may_emit(const mi_material& m) {
    if (m.kind == MI_MAT_DIELECTRIC) return false;
    return !(m.emission[0] == 0.0f && m.emission[1] == 0.0f && m.emission[2] == 0.0f);      // -0 == 0; a NaN is not
}

int compile_scene(const mi_scene_desc* d, CompiledScene* out) {
    if (d->n_objects < 0 || d->n_materials < 0 || d->n_meshes < 0 || d->n_textures < 0)
        return fail(MI_ERR_INVALID, "negative count");
    if (d->n_objects > 0 && !d->objects) return fail(MI_ERR_INVALID, "objects is NULL");
    Build b;
    int rc = materials(d, b);
    if (rc == MI_OK) rc = textures(d, b);
    b.meshes.resize((size_t)d->n_meshes); b.meshf.resize((size_t)d->n_meshes); b.mb.resize((size_t)d->n_meshes);
    for (int mi = 0; mi < d->n_meshes && rc == MI_OK; mi++) rc = mesh(d, mi, b);
    if (rc == MI_OK) rc = place_meshes(d, b);
    if (rc == MI_OK) rc = scene_objects(d, b);
    if (rc != MI_OK) return rc;
    CompiledScene& c = *out;
    c = CompiledScene();
    mesh_table(b, c);
    object_list(b);
    root_boxes(b, c);
    rotations(b);
    rc = layout(b, c);
    if (rc != MI_OK) return rc;
    c.emit = emit_flags(d, b);
    c.list = std::move(b.list);
    c.n_list_tri = b.n_list[0]; c.n_list_sphere = b.n_list[1]; c.n_unmasked = b.n_list[2] + b.n_list[3];
    c.gen_volumes = !b.bobjs.empty();
    for (const DMesh& M : b.live) if (M.material < 0 || M.tex[4] >= 0) c.mesh_maps = true;
    c.lds_bytes = (uint32_t)((b.nodes.size() + b.tris.size()) * 4);
    for (int k = 0; k < 3; k++) { c.point_light_pos[k] = d->point_light_pos[k]; c.ambient[k] = d->ambient[k]; }
    return MI_OK;
}

// The LDS image of a walker block is the head of the pools up to the last tree it walks (place_meshes puts those trees first):
//   kWalkSplit    interior and leaf records (explicit links make its interior step shorter than wf_trav's); eight 256-thread blocks
//                 per CU for the teapot.  One mesh: the clamped box test on 32-byte records, 22 VALU per step like the paired layout's,
//                 on half the LDS (cfg2 walker 22.4 against 22.8 ms)
//   kWalkPaired   the same with the interior records in the paired layout (near / far plane per axis behind one 8-byte read: no
//                 selects in the box test): four 512-thread blocks per CU = 8 waves per SIMD.  Several small meshes (the MULTI forms
//                 have no register left for the clamped form's class test)
//   kWalkInterior interior records only, leaves from global memory: two 1024-thread blocks per CU while they fit 78 KB, one up to 156 KB
//   kWalkGlobal   everything from global memory
WalkerPlan plan_walker(const CompiledScene& sc, uint32_t ref_mask, int lds_override, int bpc_override, bool global_bvh) {
    int nodes = 0, inodes = 0;
    for (size_t m = 0; m < sc.meshes.size(); m++) if (m >= 32 || ((ref_mask >> m) & 1u)) {
        nodes = std::max(nodes, sc.meshes[m].node_end); inodes = std::max(inodes, sc.meshes[m].inode_end);
    }
    const int leaves = nodes - inodes;           // the split pools hold every tree in the node pool's order
    const size_t inode_bytes = (size_t)inodes * 32;
    const size_t split_bytes = inode_bytes + (size_t)leaves * 48;
    const size_t pair_bytes = (((size_t)inodes * (size_t)kPairStride + 15) & ~(size_t)15) + (size_t)leaves * 48;
    auto fits = [&](int form) {
        switch (form) {
        case kWalkGlobal: return true;
        case kWalkInterior: return nodes > 0 && inode_bytes <= 156u * 1024u;
        case kWalkSplit: return nodes > 0 && split_bytes <= 64u * 1024u;
        case kWalkPaired: return nodes > 0 && pair_bytes <= 40u * 1024u;
        default: return false;
        }
    };
    WalkerPlan p{};
    p.form = kWalkGlobal;
    if (nodes > 0 && !global_bvh) {
        const bool one_mesh = ref_mask == 1u && sc.S.n_meshes <= 32;
        if (one_mesh && fits(kWalkSplit)) p.form = kWalkSplit;
        else if (fits(kWalkPaired)) p.form = kWalkPaired;
        else if (fits(kWalkSplit)) p.form = kWalkSplit;
        else if (fits(kWalkInterior)) p.form = kWalkInterior;
    }
    if (fits(lds_override)) p.form = lds_override;
    switch (p.form) {
    case kWalkInterior:
        p.lds_bytes = (uint32_t)inode_bytes; p.lds_nodes = (uint32_t)inodes;
        p.blocks_per_cu = inode_bytes <= 78u * 1024u ? 2 : 1;
        break;
    case kWalkSplit:
        p.lds_bytes = (uint32_t)split_bytes; p.lds_nodes = (uint32_t)inodes; p.lds_tris = (uint32_t)leaves;
        p.blocks_per_cu = std::min(8u, std::max(2u, (uint32_t)((160u * 1024u) / split_bytes)));
        break;
    case kWalkPaired:
        p.lds_bytes = (uint32_t)pair_bytes; p.lds_nodes = (uint32_t)inodes; p.lds_tris = (uint32_t)leaves;
        p.blocks_per_cu = std::min(4u, std::max(1u, (uint32_t)((160u * 1024u) / pair_bytes)));
        break;
    default:
        p.blocks_per_cu = 6;                     // bounded by 8 waves per SIMD
    }
    if (bpc_override > 0) p.blocks_per_cu = (uint32_t)bpc_override;
    return p;
}

DScene CompiledScene::device_scene(void* blob) const {
    uint8_t* p = (uint8_t*)blob;
    DScene D = S;
    D.objects = (const DObject*)(p + off.obj);
    D.list = (const DObject*)(p + off.list);
    D.bobjs = (const DObject*)(p + off.bobj);
    D.obj_rot = (const float*)(p + off.rot);
    D.materials = (const DMaterial*)(p + off.mat);
    D.meshes = (const DMesh*)(p + off.mesh);
    D.meshf = (const DMeshF*)(p + off.meshf);
    D.fnodes = (const float*)(p + off.fnodes);
    D.ftris = (const float*)(p + off.ftris);
    D.nodes = (const float*)(p + off.nodes);
    D.e2s = (const float*)(p + off.e2);
    D.inodes = (const float*)(p + off.inodes);
    D.lnodes = (const float*)(p + off.lnodes);
    D.tris = (const float*)(p + off.tris);
    D.triattr = (const DTriAttr*)(p + off.attr);
    D.textures = (const DTexture*)(p + off.tex);
    D.texels = (const uint8_t*)(p + off.texel);
    return D;
}

}  // namespace pt
