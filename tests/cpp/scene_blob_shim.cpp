// scene_blob_shim.cpp — CPU entry into the scene compiler (TEST INFRASTRUCTURE, compiled with scene_compile.cpp by
// tests/test_scene_compile_host.py into a shared object loaded with ctypes: once with g++ -ffp-contract=off, once with the
// product's host compiler and flags).  It stands in for mi_rt.cpp: it defines pt::fail, runs pt::compile_scene and hands out
// every byte and table of the result, and pt::plan_walker on it, without a GPU.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../cs397raytracingsp22_amd/csrc/scene_compile.hpp"

namespace {
char g_err[512];
}

int pt::fail(int code, const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}

// mirrored by BlobInfo in tests/test_scene_compile_host.py
struct BlobInfo {
    int32_t rc;                    // compile_scene's return code
    char err[512];                 // the recorded message of a failure
    uint64_t image_bytes;
    uint64_t off[17];              // CompiledScene::Offsets in declaration order
    // DScene: n_list_tri, n_list_sphere, n_list_plane, n_list_volume, n_list_lin, top_meshf, n_objects, n_meshes, n_nodes, n_tris, n_fnodes
    int32_t counts[11];
    int32_t n_mesh_table;          // CompiledScene::meshes
    int32_t n_list;                // CompiledScene::list
    int32_t c_n_list_tri, c_n_list_sphere, n_unmasked, mesh_maps, gen_volumes;
    uint32_t lds_bytes;
    int32_t size_of[6];            // DObject, DMaterial, DMesh, DMeshF, DTriAttr, DTexture
};

// mirrored by MeshRow
struct MeshRow { int32_t node_end, inode_end, qualifies, default_ts, cullable, pad; double corner[24]; };

// The compiled scene, or NULL with info->rc / info->err set.  Free with scene_blob_free.
extern "C" void* scene_blob_compile(const mi_scene_desc* d, BlobInfo* info) {
    g_err[0] = 0;
    memset(info, 0, sizeof *info);
    pt::CompiledScene* sc = new pt::CompiledScene();
    info->rc = pt::compile_scene(d, sc);
    snprintf(info->err, sizeof info->err, "%s", g_err);
    info->size_of[0] = (int32_t)sizeof(pt::DObject); info->size_of[1] = (int32_t)sizeof(pt::DMaterial); info->size_of[2] = (int32_t)sizeof(pt::DMesh);
    info->size_of[3] = (int32_t)sizeof(pt::DMeshF); info->size_of[4] = (int32_t)sizeof(pt::DTriAttr); info->size_of[5] = (int32_t)sizeof(pt::DTexture);
    if (info->rc != MI_OK) { delete sc; return nullptr; }
    const pt::CompiledScene::Offsets& o = sc->off;
    const size_t off[17] = { o.obj, o.list, o.bobj, o.rot, o.mat, o.mesh, o.meshf, o.fnodes, o.ftris, o.nodes, o.e2, o.inodes, o.lnodes, o.tris, o.attr, o.tex, o.texel };
    for (int k = 0; k < 17; k++) info->off[k] = off[k];
    info->image_bytes = sc->image.size();
    const pt::DScene& S = sc->S;
    const int32_t counts[11] = { S.n_list_tri, S.n_list_sphere, S.n_list_plane, S.n_list_volume, S.n_list_lin, S.top_meshf, S.n_objects, S.n_meshes, S.n_nodes, S.n_tris, S.n_fnodes };
    memcpy(info->counts, counts, sizeof counts);
    info->n_mesh_table = (int32_t)sc->meshes.size();
    info->n_list = (int32_t)sc->list.size();
    info->c_n_list_tri = sc->n_list_tri; info->c_n_list_sphere = sc->n_list_sphere; info->n_unmasked = sc->n_unmasked;
    info->mesh_maps = sc->mesh_maps ? 1 : 0; info->gen_volumes = sc->gen_volumes ? 1 : 0;
    info->lds_bytes = sc->lds_bytes;
    return sc;
}

extern "C" void scene_blob_free(void* h) { delete (pt::CompiledScene*)h; }

// image [image_bytes], rows [n_mesh_table], list [n_list * sizeof(DObject)]; any may be NULL
extern "C" void scene_blob_read(void* h, uint8_t* image, MeshRow* rows, uint8_t* list) {
    const pt::CompiledScene* sc = (const pt::CompiledScene*)h;
    if (image && !sc->image.empty()) memcpy(image, sc->image.data(), sc->image.size());
    if (rows) for (size_t m = 0; m < sc->meshes.size(); m++) {
        const pt::CompiledScene::Mesh& M = sc->meshes[m];
        MeshRow& R = rows[m];
        R.node_end = M.node_end; R.inode_end = M.inode_end; R.qualifies = M.qualifies ? 1 : 0; R.default_ts = M.default_ts ? 1 : 0;
        R.cullable = M.cullable ? 1 : 0; R.pad = 0;
        for (int k = 0; k < 8; k++) for (int r = 0; r < 3; r++) R.corner[k * 3 + r] = M.cullable ? M.corner[k][r] : 0.0;
    }
    if (list && !sc->list.empty()) memcpy(list, sc->list.data(), sc->list.size() * sizeof(pt::DObject));
}

// out: form, lds_bytes, lds_nodes, lds_tris, blocks_per_cu
extern "C" void scene_blob_plan(void* h, uint32_t ref_mask, int32_t lds_override, int32_t bpc_override, int32_t global_bvh, uint32_t* out) {
    const pt::WalkerPlan p = pt::plan_walker(*(const pt::CompiledScene*)h, ref_mask, lds_override, bpc_override, global_bvh != 0);
    out[0] = (uint32_t)p.form; out[1] = p.lds_bytes; out[2] = p.lds_nodes; out[3] = p.lds_tris; out[4] = p.blocks_per_cu;
}
