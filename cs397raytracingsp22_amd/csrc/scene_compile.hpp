// scene_compile.hpp — the scene compiler: a mi_scene_desc in, the host image of the device blob (pt_device.h layout) and
// the tables the host side of a render needs out.  Host code only: no HIP call, no context; mi_scene_upload commits the result.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mi_rt.h"
#include "pt_device.h"

#pragma clang fp contract(off)

namespace pt {

// the library's error reporter (mi_rt.cpp): records the message for mi_last_error and returns `code`
int fail(int code, const char* fmt, ...);

// host f32 math in the reference's operation order (compiled with -ffp-contract=off: the hoisted values are bit-exact)
struct h3 { float x, y, z; };
inline h3 H3(float x, float y, float z) { h3 r = { x, y, z }; return r; }
inline h3 H3p(const float* p) { return H3(p[0], p[1], p[2]); }
inline h3 sub(h3 a, h3 b) { return H3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline h3 add(h3 a, h3 b) { return H3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline h3 scale(h3 a, float s) { return H3(a.x * s, a.y * s, a.z * s); }
inline float dot(h3 a, h3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline h3 cross(h3 a, h3 b) { return H3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
inline h3 normalize(h3 a) { return scale(a, 1.0f / sqrtf(dot(a, a))); }

// May a hit of this material add light to a path?  False only when the emission the kernels would read is exactly (+-0, +-0, +-0): a NaN
// component counts as emitting, and a Dielectric never emits whatever its descriptor says (materials.rs:102: the compiler stores zeros).
bool material_may_emit(const mi_material& m);

// What wf_main's final-segment cull (pt_kernels.hip) needs to know about the scene: which entries MAY emit.  A list
// object takes the flag of its material, a ConvexVolume that of its phase material; a mesh may emit when its fixed material does or an
// emission map is bound.  Carried beside the blob, never inside it.  The kernel reads object_bits and any_mesh (mi_scene_upload: WfArgs.fin);
// the list and mesh masks are what a test order "emitters first" needs (DESIGN_HISTORY.md "Final-segment cull": built, measured, no gain).
struct EmitFlags {
    std::vector<uint32_t> object_bits;   // bit i of the array: Scene.objects entry i may emit (at least one word)
    uint64_t list_mask = 0;              // bit k: entry k of the kind-grouped list may emit; complete when list_mask_valid
    bool list_mask_valid = false;        // the list has at most 64 entries
    uint32_t mesh_mask = 0;              // bit m: live mesh m < 32 may emit
    bool any_mesh = false;               // some live mesh may emit (meshes 32, 33, ... included)
    bool any_volume = false;             // some ConvexVolume may emit
};

struct CompiledScene {
    // the blob: objects | list | boundary records | rotations | materials | meshes | F-tree meshes | F-tree nodes / triangles |
    // nodes | e2 | interior / leaf records | triangles | attributes | textures | texels, each pool 256-byte aligned
    std::vector<uint8_t> image;
    struct Offsets { size_t obj, list, bobj, rot, mat, mesh, meshf, fnodes, ftris, nodes, e2, inodes, lnodes, tris, attr, tex, texel; } off{};
    DScene S{};                       // counts and list parameters; the pool pointers are set by device_scene
    // per live mesh (Scene.objects order): end of its tree in the node pool and in the interior-record pool (the walked trees are
    // placed first, so the LDS window of a walker is a head of the pool), does the two-stage bound apply to it at all, is it walked
    // two-stage by default (qualifies and large enough for the F-tree to pay), and the world-space corners of its root box (tile masks)
    struct Mesh { int node_end, inode_end; bool qualifies, default_ts, cullable; double corner[8][3]; };
    std::vector<Mesh> meshes;
    std::vector<DObject> list;        // the kind-grouped list as the kernels read it (tile masks: its Triangles and Spheres)
    int n_list_tri = 0, n_list_sphere = 0, n_unmasked = 0;   // planes + volumes: never masked
    EmitFlags emit;                   // may-emit flags of the objects, the list positions and the live meshes
    bool mesh_maps = false;           // some mesh takes its material from maps or has a normal map: wf_main's MESH = 2 form
    bool gen_volumes = false;         // a ConvexVolume whose boundary is not the inline sphere: the kernels' GV forms
    uint32_t lds_bytes = 0;           // bytes needed to stage nodes + tris (the K1 megakernels), 0 = no meshes
    float point_light_pos[3] = { 0.0f, 1.0f, 5.0f }, ambient[3] = { 0.1f, 0.1f, 0.1f };   // Scene fields read by Phong

    // S with its pool pointers into a device copy of `image` at `blob`
    DScene device_scene(void* blob) const;
};

// MI_OK, or the error code with its message recorded (fail); `out` is complete only on MI_OK
int compile_scene(const mi_scene_desc* d, CompiledScene* out);

// How a render walks the meshes of ref_mask (bit m = live mesh m; meshes 32, 33, ... are always included) through the reference's
// tree.  lds_override: MI_RT_WF_TRAV_LDS (-1 = automatic; a form whose image does not fit is ignored), bpc_override: MI_RT_WF_TRAV_BPC
// (0 = automatic), global_bvh: MI_RT_GLOBAL_BVH (the automatic choice keeps every tree in global memory).
WalkerPlan plan_walker(const CompiledScene& sc, uint32_t ref_mask, int lds_override, int bpc_override, bool global_bvh);

}  // namespace pt
