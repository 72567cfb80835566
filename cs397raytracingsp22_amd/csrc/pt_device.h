// pt_device.h — device-resident scene layout shared by the host scene compiler
// (scene_compile.cpp) and the HIP kernels (pt_kernels.hip).  gfx950 only.
//
// Layout rules (DESIGN.md "Data layout in HBM"):
//  * The linear object list of Scene.objects (tracing.rs:215,330) is an array of
//    fixed 64-byte records read at a wave-uniform index, so every lane of a wave
//    reads the same record and the compiler serves it with scalar (SMEM) loads.
//  * Each mesh BVH (reference topology, geometry.rs:190-217) is stored THREADED in
//    DFS pre-order: node i's left child is i+1 and `skip` is the node that follows i's
//    subtree.  The reference always descends left-then-right (geometry.rs:105-115),
//    so a skip link replaces the traversal stack exactly.
//  * Nodes are 2 x float4 (32 B), triangles 3 x float4 (a, e1, e2 — 48 B) so a lane
//    fetches a node / triangle with 16-byte loads from LDS or L1/L2.  Leaf nodes hold {a, skip}{e1, tri} (see DScene.e2s).
//  * Per-triangle shading attributes (normals, uvs, tangent) are a separate array
//    touched once per mesh HIT, not per candidate.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

// Read-only scene data is typed as CONSTANT address space on the device: a read at a
// wave-uniform address then compiles to a scalar (SMEM) load into SGPRs even when the kernel
// also stores to global memory (with plain global pointers the compiler must assume the
// stores may alias and falls back to per-lane vector loads).  Same 8-byte pointers on the host.
#if defined(__HIP_DEVICE_COMPILE__)
#define PT_CONST_AS __attribute__((address_space(4)))
#else
#define PT_CONST_AS
#endif

namespace pt {

constexpr int kTile = 32;            // MI_TILE
constexpr int kTilePixels = kTile * kTile;
constexpr int kBlock = 256;          // threads per workgroup = 4 waves of 64
constexpr int kBlocksPerTile = kTilePixels / kBlock;

enum : int { OBJ_SPHERE = 0, OBJ_TRIANGLE = 1, OBJ_PLANE = 2, OBJ_VOLUME = 3, OBJ_MESH = 4 };
enum : int { MAT_LAMBERTIAN = 0, MAT_METAL = 1, MAT_DIELECTRIC = 2, MAT_PARAMETERIZED = 3, MAT_ISOTROPIC = 4 };

// One entry of Scene.objects, 16 words.  Word use by kind:
//   SPHERE   f[0..2] center, f[3] radius, f[4] radius*radius
//   TRIANGLE f[0..2] a, f[3..5] e1=b-a, f[6..8] e2=c-a, f[9..11] normalize(e1 x e2)
//   PLANE    f[0..2] point, f[3..5] normal
//   VOLUME   f[0..2] boundary center, f[3] radius, f[4] radius*radius, f[5] -1/density; ref = -1: that inline sphere is the boundary,
//            else ref = first of int(f[6]) boundary records in DScene.bobjs (a Triangle / Plane / StaticMesh, or a nested Scene's entries)
//   MESH     ref = mesh index
// Every derived value is computed on the host with the same f32 operation the
// reference performs per ray (geometry.rs:400,434-435,449,517), so hoisting it is exact.
struct alignas(16) DObject {
    int32_t kind;
    int32_t material;    // material index (phase function for VOLUME); unused for MESH
    int32_t ref;         // mesh index for MESH
    int32_t index;       // position in Scene.objects (used by the kind-grouped `list` copy)
    float   f[12];
};
static_assert(sizeof(DObject) == 64, "DObject must be 64 bytes");

// Material, 16 words: kind, albedo, emission, roughness, metallic, ior, albedo/PI
struct alignas(16) DMaterial {
    int32_t kind;
    float   albedo[3];
    float   emission[3];
    float   roughness;
    float   metallic;
    float   ior;
    float   albedo_over_pi[3];   // materials.rs:41,128 `self.albedo / PI`, hoisted (exact: same f32 division)
    float   pad[3];
};
static_assert(sizeof(DMaterial) == 64, "DMaterial must be 64 bytes");

struct DTexture {
    uint32_t offset;     // byte offset of the RGB8 texels in the texel pool
    int32_t  width;
    int32_t  height;
    int32_t  pad;
};

// StaticMesh (geometry.rs:127-134)
struct alignas(16) DMesh {
    float    transform[16];      // column-major
    float    inv_transform[16];  // column-major
    int32_t  node_begin;         // index of the root node in the node pool
    int32_t  node_end;           // one past the last node of this mesh
    int32_t  tri_begin;          // first triangle in the triangle pools
    int32_t  n_tris;
    int32_t  material;           // -1 = ParameterizedMaterial from textures
    int32_t  tex[5];             // -1 = None
    int32_t  object_index;       // position in Scene.objects (tie-breaking)
    int32_t  e2_begin;           // first entry of this mesh in the e2 pool (leaf-embedded triangles, see DScene.e2s)
    // When all the maps this mesh binds have the same size, their texels are ALSO stored interleaved, 16 bytes per texel:
    // {albedo.rgb, metallic.x}{emission.rgb, roughness.x}{normal.rgb, 0}{0}: one 16-byte fetch per hit instead of up to five
    // 4-byte fetches from five different cache lines (incoherent rays: every fetch is a line of its own).  Same bytes, same
    // (float)b / 255 conversions, same texel index -> same values.  -1 = not available (sizes differ / fixed material).
    int32_t  tex_comb;           // index into DScene.textures of the interleaved array
    int32_t  i_root;             // id of this mesh's root in the split pools (DScene.inodes / lnodes): >= 0 interior record, < 0 = ~leaf record
    int32_t  pad2[2];
};
static_assert(sizeof(DMesh) % 16 == 0, "DMesh must be 16-byte sized");

// Two-stage traversal data of a StaticMesh (bvh_build.hpp FTree): where its F-tree lives and the constants of the
// per-ray padding bound.  qualifies = 0: the bound never applies to this mesh (object-space scale makes the reference's
// absolute 1e-4 determinant test void) and it is always walked through the reference's own tree.
struct alignas(16) DMeshF {
    int32_t fnode_begin, fnode_end;   // this mesh's F-nodes in the F-node pool
    int32_t ftri_begin;               // first entry of this mesh in the F-ordered triangle pool
    int32_t qualifies;
    float   E2, L;                    // max |e1||e2|, longest stored edge
    float   cx, cy, cz, R;            // bounding sphere of the vertices (object space)
    float   pad[2];
    float   qs, qbx, qby, qbz;        // grid of the quantised F-nodes: coordinate = fmaf(q, qs, qb) (bvh_build.hpp fq_encode)
};
static_assert(sizeof(DMeshF) == 64, "DMeshF must be 64 bytes");

// per-triangle shading attributes, 20 floats = 5 float4
struct alignas(16) DTriAttr {
    float na[3], nb[3], nc[3];   // corner normals          geometry.rs:350
    float ta[2], tb[2], tc[2];   // corner uvs              geometry.rs:355
    float tan[3];                // StaticMesh::get_tangent geometry.rs:245-250, hoisted (exact)
    float pad[2];
};
static_assert(sizeof(DTriAttr) == 80, "DTriAttr must be 80 bytes");

struct DScene {
    const PT_CONST_AS DObject*   objects;
    const PT_CONST_AS DMaterial* materials;
    const PT_CONST_AS DMesh*     meshes;
    const PT_CONST_AS float*     nodes;      // float4 pairs: {bmin.xyz, skip(int)} {bmax.xyz, tri(int, -1 = interior)}
    const PT_CONST_AS float*     tris;       // float4 triples: {a.xyz, 0} {e1.xyz, 0} {e2.xyz, 0}
    // LEAF nodes carry their triangle instead of a box (the reference never box-tests a leaf, geometry.rs:95, so no
    // kernel reads a leaf's box): {a.xyz, skip}{e1.xyz, tri}; the third operand comes from this pool, float4 {e2.xyz, 0} per
    // triangle, ordered like the node pool.  A walker that has just fetched a leaf node from LDS then needs ONE more
    // 16-byte LDS read for the triangle test — no trip to global memory inside the walk.
    const PT_CONST_AS float*     e2s;
    // The same trees once more with interior nodes and leaves in SEPARATE pools, every link explicit (wf_trav_i: only the
    // interior records are staged in LDS — half the bytes, so a tree that needs one 1024-thread block per CU as a whole image
    // runs two of them).  A link is an id: >= 0 = interior record, < 0 = ~(leaf record), kIdEnd = the walk of this mesh is over.
    //   inodes: float4 pairs {bmin.xyz, id on a miss (skip link)}{bmax.xyz, id on a hit (left child)}
    //   lnodes: float4 triples {a.xyz, id of the next node}{e1.xyz, triangle index}{e2.xyz, 0}
    const PT_CONST_AS float*     inodes;
    const PT_CONST_AS float*     lnodes;
    const PT_CONST_AS DTriAttr*  triattr;
    const PT_CONST_AS DTexture*  textures;
    const PT_CONST_AS uint8_t*   texels;
    // the non-mesh objects again, GROUPED BY KIND (triangles, spheres, planes, volumes; stable
    // within a kind), each record carrying its Scene.objects index: the hit loop runs one
    // tight loop per kind with no per-object dispatch.  Exact: the closest hit is order
    // independent, ties go to the lower Scene.objects index (tracing.rs:335), and only
    // volumes draw random numbers, in their original relative order (geometry.rs:517).
    const PT_CONST_AS DObject*   list;
    // boundary records of ConvexVolumes whose boundary is not the inline sphere (same record format; MESH: ref = entry of `meshes`
    // at or behind n_meshes — the table holds the Scene.objects meshes first, then the boundary-only ones)
    const PT_CONST_AS DObject*   bobjs;
    // sample_hemisphere's rotation for the two normals of every list Triangle, hoisted to the host (scene_compile.cpp): 3 float4 per entry,
    // entry 2 i + (frontface ? 0 : 1) of Scene.objects entry i
    const PT_CONST_AS float*     obj_rot;
    // two-stage traversal (meshes that qualify): F-tree nodes QUANTISED to 16 bytes (bvh_build.hpp fq_encode: three words of 16-bit box
    // faces on the mesh's grid DMeshF.qs / qb, then the link: the skip index of an interior node, 0x80000000 | (first << 3) | (count - 1)
    // into ftris for a leaf), the F-ordered triangles {a.xyz, tri index}{e1.xyz, 0}{e2.xyz, 0}, and the per-mesh constants
    const PT_CONST_AS float*     fnodes;
    const PT_CONST_AS float*     ftris;
    const PT_CONST_AS DMeshF*    meshf;
    int32_t n_list_tri, n_list_sphere, n_list_plane, n_list_volume;
    // Top-level tree over the list's Triangles (long lists only): the first n_list_lin Triangles of `list` (the large
    // ones) are tested one by one, the others sit in a padded SAH tree whose record is meshf[top_meshf] (the F-tree machinery of the
    // two-stage mesh traversal, in world space); top_meshf = -1: no tree, n_list_lin = n_list_tri
    int32_t n_list_lin, top_meshf;
    int32_t n_objects;
    int32_t n_meshes;
    int32_t n_nodes;
    int32_t n_tris;
    int32_t n_fnodes;
};

// Camera::generate_rays constants (tracing.rs:160-163,187-191), computed once on the
// host with the reference's f32 operations.
struct DCamera {
    float eye[3];
    float rot[9];          // Matrix3::from_cols(normalize(view x up), up, -view), column-major
    float pixel_size;      // 1 / H
    float n;               // aa_sample_count as f32
    float rootn;           // sqrt(n)
    float half_rootn;      // 0.5 * rootn
    float half_n;          // 0.5 * n
    float cx_base;         // -0.5*W   (x as f32 + cx_base + 0.5)
    float cy_base;         // 0.5 + 0.5*H
    float focal_length;
    float focus_dist;
    float lens_radius;
    float max_trace_dist;
    uint32_t rootn_u;      // rootn as u32
    uint32_t spp;          // aa_sample_count
    uint32_t zone;         // rand UniformInt rejection zone for range = spp
    uint32_t path_depth;
    uint32_t width, height;
    // CameraProjectionMode::Orthographic (tracing.rs:196,200,204): origin = (centre.x, centre.y, 0) in
    // camera space as it is, direction = rot * view_dir (the constant, rotated once on the host)
    uint32_t ortho;
    float ortho_dir[3];
    // ShadingMode::Phong (tracing.rs:277-297): Scene.point_light_pos / ambient
    float light[3];
    float ambient[3];
};

struct DRender {
    uint32_t seed;
    int32_t  rank, world;
    uint32_t tiles_x, tiles_y, tiles_total;
    uint32_t my_tiles;       // tiles owned by this rank
    uint32_t lds_nodes;      // number of BVH nodes staged into LDS (0 = read from global)
    uint32_t lds_tris;       // number of triangles staged into LDS
    uint32_t vote_t, vote_a; // VOTED kernel: run the BVH phase when n_trav*vote_t >= n_a*vote_a
    uint32_t k_steps;        // VOTED kernel: node micro-steps per BVH trip
};

// kernel argument block of K1 (passed by value: lives in the kernarg segment / SGPRs)
struct K1Args {
    DScene  S;
    DCamera C;
    DRender R;
    uint32_t seed_key;   // lowbias32(seed ^ 0x68e31da4)
    float*    out;       // [tiles_padded][1024][3]
    uint32_t* sig;       // [tiles_padded][1024] or nullptr
    unsigned long long* diag;   // 16 counters (diagnostic build only) or nullptr
};

// ---- ray queries (pt_kernels.hip rq_intersect / rq_shade): caller-supplied rays, one lane per ray ----
// Ray i of the batch draws from the stream (seed, first_key + i, 0).  Every out_* of RqArgs except out_object may be nullptr.
struct RqArgs {
    DScene  S;
    uint32_t lds_nodes, lds_tris;    // as DRender: BVH nodes / triangles staged into LDS (0 = read from global memory)
    uint32_t seed_key;               // lowbias32(seed ^ 0x68e31da4)
    uint32_t first_key;
    uint32_t n_rays;
    float    t_min, t_max;
    const float* origins;            // [n][3]
    const float* dirs;               // [n][3], used as given (not normalised)
    int32_t*  out_object;            // [n] index into Scene.objects, -1 = no hit
    float*    out_distance;          // [n]
    float*    out_hitpoint;          // [n][3]
    float*    out_normal;            // [n][3]
    int32_t*  out_flags;             // [n] bit 0 frontface, bit 1 has_tex_coords
    float*    out_uv;                // [n][2]
    uint32_t* out_material;          // [n][10] words of mi_material
};
// rq_occluded (mi_occluded_rays): the any-hit query.  ray_t_max, when given, replaces t_max ray by ray.
struct RqOccArgs {
    DScene  S;
    uint32_t lds_nodes, lds_tris;
    uint32_t seed_key, first_key, n_rays;
    float    t_min, t_max;
    const float* origins;            // [n][3]
    const float* dirs;               // [n][3], used as given (not normalised)
    const float* ray_t_max;          // [n] or nullptr
    uint8_t* out_occluded;           // [n] 0 / 1
};
// rq_hemi (mi_hemisphere_occlusion): the rays are made on the device.  A group of 1 << group_log2 lanes owns one point; sample
// s = first_sample + k of point i takes its direction from the stream (seed, first_key + i, 2s) and its ray draws from (.., 2s + 1).
struct RqHemiArgs {
    DScene  S;
    uint32_t lds_nodes, lds_tris;
    uint32_t seed_key, first_key, n_points;
    uint32_t first_sample, n_samples;
    uint32_t group_log2;             // G = min(64, next_pow2(n_samples)) as a shift
    uint32_t world_radius;           // MI_HEMI_WORLD_RADIUS: the upper end is t_max / |d|
    float    t_min, t_max;
    const float* points;             // [n][3]
    const float* normals;            // [n][3], used as given (not normalised)
    uint32_t* out_open;              // [n] samples not occluded
    float*    out_bent;              // [n][3] sum of their directions, or nullptr
};
struct RqShadeArgs {
    DScene  S;
    uint32_t seed_key, first_key, n_rays;
    uint32_t path_depth, path_samples;
    float    max_trace_dist;
    const float* origins;
    const float* dirs;
    float*   out_rgb;                // [n][3]
};

// ---- wavefront pipeline (pt_kernels.hip "K1w") ----
// Path state streamed through HBM as 6 float4 planes [6][cap] (coalesced 16-byte accesses):
//   q0 o.xyz d.x | q1 d.yz T.xy | q2 T.z L.xyz | q3 rng.s0 rng.s1 pix sample|depth<<16
//   plane-4 array: packed sub-arrays {t, obj} 8 B x cap | tri 4 B x cap (class B only) | signature 4 B x cap; q5 best.u best.v mesh
constexpr int kWfPlanes = 6;
// Appends are SHARDED: block b of wf_main appends its survivors to region (b % kWfShards) of
// st_out with that shard's own counter, so no single address sees more than ~1/256 of the
// atomics (one word saturates at ~88 atomics/us on gfx950).  A shard's region can never
// overflow: it receives at most the paths its own input blocks hold.
constexpr int kWfShards = 256;
constexpr int kCandMax = 8;          // two-stage: candidate slots per queued ray (more passing triangles -> reference walk for that mesh)
constexpr int kTwoStageMaxMeshes = 24;   // mesh index bits in cand_hdr
// The header of a pass as wf_prefix stores it into the host's pinned ring slot (kHdrSlotWords words; kHdrSeq is written last,
// behind a system-scope fence, and is what the host polls)
constexpr int kHdrBlocks = 0;        // blocks of the next pass
constexpr int kHdrLive = 1;          // live paths
constexpr int kHdrQueue = 2;         // queue length (the class-B paths: the walkers' work list)
constexpr int kHdrSeq = 3;           // sequence number of the pass
constexpr int kHdrLiveB = 4;         // class-B paths (statistics only)
constexpr int kHdrBlocksA = 5;       // the class-A blocks, which come first
constexpr int kHdrSegments = 6;      // Scene::intersect_ray evaluations of the pass (statistics only)
constexpr int kHdrSlotWords = 8;
constexpr int32_t kIdEnd = (int32_t)0x80000000;   // split pools: "no further node"
constexpr int kPairStride = 56;                    // wf_trav_i<.., PAIR>: bytes of an interior record in the paired LDS layout (pt_kernels.hip)
enum : uint32_t { kFinMeshEmit = 1u };   // WfArgs.fin[0]
struct WfArgs {
    DScene  S;
    DCamera C;
    DRender R;
    uint32_t seed_key;
    float4* st_in;        // state of the live paths of the previous iteration (nullptr at iteration 0)
    float4* st_out;       // state of the paths that continue, compacted per shard region
    uint32_t cap;         // plane stride = kWfShards * region
    uint32_t region;      // slots per shard region (multiple of 256)
    uint32_t n_in;        // iteration 0: number of new paths (npix * s_count)
    uint32_t n_blocks_in; // iteration > 0: blocks to run = sum over shards of ceil(count/256)
    uint32_t part;        // a pass after the first may be launched in two parts: 0 = all blocks, 1 = the class-A blocks only, 2 = the class-B blocks
                          // only.  The grid may be larger than the part (a host-side upper bound): surplus blocks return at once
    uint32_t iter0;       // 1 = generate camera rays (first iteration of a batch)
    uint32_t s_base;      // first sample index of this batch
    uint32_t s_count;     // samples per pixel in this batch
    uint32_t npix;        // tile-major pixels of this rank = tiles_padded * 1024
    uint32_t refill_min;  // wf_trav: refill idle lanes only when at least this many are idle (amortises the gather latency)
    uint32_t fuse_max;    // wf_main: at most this many further shade + intersect rounds inside one launch ...
    uint32_t fuse_min;    // ... each taken only while at least this many lanes of the wave can continue
    // Every shard region is filled from BOTH ENDS: class A (the next shade is a plain Triangle /
    // Plane hit: the common, cheap case) grows from the front, class B (sphere hits, rays waiting
    // for a mesh walk, volumes) from the back; A + B can never exceed the region.  The next pass
    // runs all A blocks, then all B blocks, so most waves execute one shading branch only.
    const PT_CONST_AS uint32_t* in_count;    // [2*kWfShards] live paths per (class, shard) of st_in: A shards, then B shards
    const PT_CONST_AS uint32_t* in_blkpfx;   // [2*kWfShards + 1] exclusive prefix of ceil(count/256)
    uint32_t* out_count;  // [2*kWfShards] appended to st_out per (class, shard)
    uint32_t* trav_count; // [kWfShards] statistics: path segments (Scene::intersect_ray evaluations) wf_main ran, per output shard; summed and zeroed by wf_prefix.  trav_head sits behind it
    uint32_t* trav_head;  // [0]: consumption head over the CONCATENATED per-shard queues (wf_trav grabs 256 entries per atomic); [1]: the same for wf_trav_f
    const PT_CONST_AS uint32_t* trav_pfx;   // [kWfShards + 1] exclusive prefix of the class-B counts (statistics)
    const PT_CONST_AS uint32_t* hdr;   // [4] written by wf_prefix after every wf_main: blocks of the next pass, live paths, class-B paths (the walkers' work list)
    float4* samp;         // [s_count][npix] finished samples: L.xyz, signature bits
    float4* accum;        // [npix] running per-pixel sum (xyz) and signature sum (w bits)
    float*    out;        // compact framebuffer [tiles_padded][1024][3]
    uint32_t* sig;        // or nullptr
    // Primary rays only: bit k of tile_mask[global tile] = entry k of the kind-grouped list can be hit by a
    // camera ray of that 32x32 tile (conservative host-side frustum test; nullptr = test everything).
    // tile_mask[tiles_total + tile]: low 32 bits = the same for the meshes' root boxes, bit 63 = nothing
    // at all is reachable from this tile.
    const PT_CONST_AS unsigned long long* tile_mask;
    // mesh walks: bit m of trav_mask = mesh m is walked by THIS launch (wf_trav: the meshes walked through the reference's
    // tree; wf_trav_f / wf_replay: the two-stage meshes).  Results of successive launches merge through the hit record.
    uint32_t trav_mask;
    // two-stage: candidates of queue entry vi = cand[vi * kCandMax .. ) as {t, (mesh << 24) | triangle}; cand_hdr[vi] =
    // {position of the path in st_out, count | bit (8 + m): mesh m must take the reference walk (overflow, bound not applicable)}
    uint2* cand;
    uint2* cand_hdr;
    // Final-segment cull (wf_main, SIG = false forms; scene_compile.hpp EmitFlags): nullptr = off.  fin[0] = flags (kFinMeshEmit: some mesh of
    // the scene may emit), then one bit per Scene.objects entry: bit i % 32 of fin[1 + i / 32] = entry i may emit.
    const PT_CONST_AS uint32_t* fin;
    unsigned long long* diag;   // developer builds with -DPT_WF_STAMPS: [16] summed s_memtime deltas of sampled wf_main waves
    // Ray-table rendering (mi_render_rays): the camera pass takes sample s of pixel (x, y) from ray_o / ray_d at
    // ((row * height + y) * width + x) * 3, row = s when rays_per_pixel == aa_sample_count, 0 when it is 1.  nullptr = Camera::generate_rays.
    const float* ray_o;
    const float* ray_d;
    uint32_t rays_per_pixel;
    // Point-table rendering (mi_render_points): the camera pass takes the surface point and the normal of sample s of pixel (x, y) from
    // pt_p / pt_n at the same index (row = s when pt_rows == aa_sample_count, 0 when it is 1) and draws the direction itself:
    // sample_hemisphere(normal) on the stream (seed, W H + y W + x, s).  A zero normal is an empty texel.  nullptr = no point table.
    uint32_t pt_rows;
    const float* pt_p;
    const float* pt_n;
    // Light probes (mi_render_probes): pt_probes != 0 makes pt_p a table of probe positions without normals (pt_n is nullptr): the camera
    // pass draws a full-sphere direction, rand_sphere_vec on the direction stream above (the PROBES form of wf_main).  sh, or nullptr:
    // [npix][9][3] running SH L2 sums in the compact tile-major layout, which wf_reduce_sh advances behind wf_reduce in every batch.
    // A point table (pt_probes == 0) with sh (mi_render_points_sh): the same sums over the POINTS form's hemisphere directions, which
    // wf_reduce_psh advances instead (it reads pt_n and pt_rows again); never together with m2.
    uint32_t pt_probes;
    float* sh;
    // Second moments of a point-table bake (mi_render_points_moments): m2, or nullptr: [npix][3] running sums of squares of the samples in
    // the compact tile-major layout, which wf_reduce_m2 advances behind wf_reduce in every batch (never together with sh).
    float* m2;
};

constexpr int kShFloats = 27;        // one probe's SH L2 record: 9 coefficients x 3 colour channels

// How a render walks the meshes that take the reference's tree (scene_compile.cpp plan_walker -> pt_kernels.hip launch_walker).
// The form values are those of MI_RT_WF_TRAV_LDS.
enum : int {
    kWalkGlobal = 0,      // wf_trav: the tree in global memory
    kWalkInterior = 4,    // wf_trav_i<1024>: interior records in LDS, leaf records from global memory
    kWalkSplit = 5,       // wf_trav_i<256, .., LEAF_LDS>: interior and leaf records in LDS
    kWalkPaired = 6,      // wf_trav_i<512, .., LEAF_LDS, PAIR>: the same with 56-byte paired interior records
};
struct WalkerPlan {
    int form;
    uint32_t lds_bytes;       // dynamic LDS per block
    uint32_t lds_nodes;       // DRender.lds_nodes: interior records staged
    uint32_t lds_tris;        // DRender.lds_tris: leaf records staged behind them
    uint32_t blocks_per_cu;
};

// ---- lightmap atlas (mi_lightmap_texels; pt_kernels.hip "lm_*") ----
// A single-index triangle mesh's uv atlas rasterised into the point and normal tables of mi_render_points.  Triangles are binned to
// kTile x kTile-texel tiles (lm_bin counts, lm_scan sums, lm_bin fills), then lm_resolve runs one block per tile.
// Scratch: counts[tiles] cursors[tiles] (u32, zeroed per call) offsets[tiles + 1] (u64) and list[cap] (u32).  A tile whose list does not
// lie inside [0, cap) is resolved by testing every triangle of the mesh instead: cap changes the speed, never the result.
struct LmArgs {
    const float*    positions;       // [n_vertices][3]
    const float*    normals;         // [n_vertices][3]
    const float*    texcoords;       // [n_vertices][2]
    const uint32_t* indices;         // [n_triangles][3]
    uint32_t n_vertices, n_triangles;
    uint32_t width, height, rows;
    uint32_t jitter;                 // MI_LM_JITTER: row r of texel (x, y) draws (jx, jy) from the stream (seed, 2 W H + y W + x, r)
    uint32_t seed_key;
    uint32_t tiles_x, tiles_y;
    double   m[12];                  // mi_mesh.transform, rows of its upper 3 x 4, promoted to f64
    double   nm[9];                  // inverse transpose of its upper 3 x 3, row-major, computed in f64
    double   offset;
    uint32_t* counts;
    uint32_t* cursors;
    unsigned long long* offsets;
    uint32_t* list;
    unsigned long long cap;
    unsigned long long* host_total;  // pinned, device-mapped: the sum of the counts, for sizing the list
    float*   out_points;             // [rows][H][W][3]
    float*   out_normals;            // [rows][H][W][3]
    int32_t* out_triangle;           // [rows][H][W] or nullptr
};

// ---- lightmap finishing (mi_lightmap_finish; pt_kernels.hip "lmf_*") ----
// One pass of tracing.py lightmap_finish: lmf_mask (the covered mask from the normals, and the masked copy when there is no other pass),
// lmf_atrous (one filter level, step `step`, one kTile x kTile tile per block) or lmf_dilate (one dilation pass).  Every pass reads `src`
// (and `mask_in`) and writes `dst` (and `mask_out`): ping-pong, never in place.
struct LmfArgs {
    const float*   src;              // [H][W][3] the previous pass's image
    const float*   points;           // [H][W][3] guides (lmf_atrous)
    const float*   normals;          // [H][W][3] guides: all-zero = empty texel
    float*         dst;              // [H][W][3]
    const uint8_t* mask_in;          // [H][W] lmf_dilate: the previous pass's valid mask
    uint8_t*       mask_out;         // [H][W] lmf_mask, lmf_dilate
    uint32_t width, height, tiles_x, tiles_y;
    uint32_t step;                   // lmf_atrous: s = 2^level
    uint32_t npow;                   // normal_power_log2
    uint32_t copy;                   // lmf_mask: also write dst = covered ? src : +0
    float sigma_plane, reach, sigma_color;
};
// Largest step whose tile plus 2 s halo (9 planes of (kTile + 4 s)^2 f32) fits the CU's 160 KiB of LDS
constexpr uint32_t kLmfMaxLdsStep = 8;
inline size_t lmf_lds_bytes(uint32_t step) { const size_t e = (size_t)kTile + 4u * step; return 9u * e * e * sizeof(float); }

// ---- directional lightmaps (mi_lightmap_finish_sh, mi_lightmap_sh_eval; pt_kernels.hip "lsh_*") ----
// tracing.py lightmap_finish_sh: lmf_mask<27>, lsh_atrous and lmf_dilate<27> are lmf_mask, lmf_atrous' direct form and lmf_dilate for images of
// [H][W][9][3] records; they take LmfArgs with src and dst holding kShFloats floats per texel.  lsh_eval is tracing.py lightmap_sh_eval:
struct LshEvalArgs {
    const float* sh;                 // [n][9][3]
    const float* normals;            // [n][3]: all-zero = empty texel, +0.0
    float*       out_irradiance;     // [n][3]
    uint32_t     n;
};

// ---- lightmap lookup (mi_lightmap_sample, mi_lightmap_sh_sample; pt_kernels.hip "lml_*") ----
// tracing.py lightmap_sample (lml_sample<3>, lml_sample<27>) and lightmap_sh_sample (lml_sh_sample): one lane per uv point
// (the texels are f32 for the lml_* kernels and packed for the lmp_* ones below: the kernel's texel-fetch policy knows which)
struct LmlArgs {
    const void*    image;            // [H][W][C]: C = 3 or 27 (lml_sample<C>), 27 (lml_sh_sample)
    const uint8_t* valid;            // [H][W] or nullptr = all valid: 0 = the texel takes no part and is not read
    const float*   uv;               // [n][2]
    const float*   normals;          // [n][3] (lml_sh_sample): all-zero = +0.0 and weight 0
    float*         out;              // [n][C] (lml_sample<C>), [n][3] (lml_sh_sample)
    float*         out_weight;       // [n] or nullptr
    uint32_t width, height, n;
    uint32_t nearest;                // MI_LS_NEAREST
};

// ---- lightmap mips (mi_lightmap_mips, mi_lightmap_sample_lod, mi_lightmap_sh_sample_lod; pt_kernels.hip "lmm_*", "lml_*_lod") ----
// The layout is render_plan.cpp mip_plan's: levels 1 .. L - 1 tightly one after the other, offsets in texels.
constexpr uint32_t kMipMaxLevels = 16;   // the full chain of 32768 texels
constexpr uint32_t kMipFuse = 5;         // the levels one launch of lmm_reduce writes from a 32 x 32 tile: 16, 8, 4, 2, 1 squared
// tracing.py lightmap_mips (lmm_reduce<3>, lmm_reduce<27>): one block per 32 x 32 tile of the level read, `count` levels written
struct LmmArgs {
    const float*   src;              // the level read, [src_h][src_w][C]
    const uint8_t* src_valid;        // level 0 only: [H][W] or nullptr = all valid
    const float*   src_cov;          // levels >= 1: the coverage of the level read; nullptr: level 0, whose coverage is its mask's
    float*         mips;             // levels 1 .. L - 1, tightly: [texels][C]
    uint8_t*       mip_valid;        // [texels] or nullptr
    float*         mip_cov;          // [texels]
    uint64_t       off[kMipFuse];    // where the levels written start, in texels
    uint32_t src_w, src_h, count, tiles_x;
};
// tracing.py lightmap_sample_lod (lml_sample_lod<3>, lml_sample_lod<27>) and lightmap_sh_sample_lod (lml_sh_sample_lod): one lane per point
struct LmlLodArgs {
    const void*    image;            // level 0, [H][W][C]
    const uint8_t* valid;            // level 0's mask or nullptr = all valid
    const void*    mips;             // levels 1 .. L - 1 (nullptr when levels == 1)
    const uint8_t* mip_valid;        // their masks or nullptr = every texel of every level valid
    const float*   uv;               // [n][2]
    const float*   lod;              // [n]
    const float*   normals;          // [n][3] (lml_sh_sample_lod)
    float*         out;              // [n][C] (lml_sample_lod<C>), [n][3] (lml_sh_sample_lod)
    float*         out_weight;       // [n] or nullptr
    uint64_t       off[kMipMaxLevels];                        // level l starts at texel off[l] of mips (off[0] unused)
    uint32_t       lw[kMipMaxLevels], lh[kMipMaxLevels];      // the levels' sizes
    uint32_t levels, n;
    uint32_t       boff[kMipMaxLevels];                       // BC6H texels only: level l starts at block boff[l] of mips (else unused)
};

// ---- packed lightmaps (mi_lightmap_pack, mi_lightmap_unpack, mi_lightmap_*_packed; pt_kernels.hip "lmp_*") ----
// The storage formats (MI_LP_*): f16 texels are `channels` u16 each, tightly; an RGB9E5 texel is one u32 (3 channels only).  Both decode
// to f32 exactly, so a packed lookup is the lml_* device code with another texel-fetch policy and takes LmlArgs / LmlLodArgs as they are.
constexpr uint32_t kLpF16 = 1, kLpRgb9e5 = 2;
// tracing.py lightmap_pack (lmp_pack<F>) and lightmap_unpack (lmp_unpack<F>): one lane per pair of f16 elements or per RGB9E5 texel
struct LmpArgs {
    const void* src;                 // pack: [n] f32; unpack: [n] packed items
    void*       dst;                 // pack: [n] packed items; unpack: [n] f32
    uint64_t    n;                   // f16: elements (texels x channels); RGB9E5: texels (three floats each)
};

// ---- BC6H lightmaps (mi_lightmap_bc6h_encode, mi_lightmap_bc6h_decode, mi_lightmap_sample_bc6h; pt_kernels.hip "lmb_*") ----
// BC6H_UF16 blocks of the one mode tracing.py lightmap_bc6h_encode writes: 16 bytes per 4 x 4 texels, ceil(W / 4) x ceil(H / 4) blocks,
// row-major (render_plan.cpp bc6h_plan).  A BC6H lookup is the lml_* device code with the texel-fetch policy LmTexBc6h; kLpBc6h names
// it beside kLpF16 and kLpRgb9e5 inside the library only (the MI_LP_* calls refuse it: the format is lossy and has its own entry points).
constexpr uint32_t kLpBc6h = 3;
constexpr uint32_t kBc6hMaxRounds = 4;
// tracing.py lightmap_bc6h_encode (lmb_encode: one lane per texel, or lmb_encode_block: one lane per block) and lightmap_bc6h_decode
// (lmb_decode: one lane per texel)
struct LmbArgs {
    const float*   image;            // encode: [H][W][3] f32
    const uint8_t* valid;            // encode: [H][W] or nullptr = every texel takes part
    void*          blocks;           // [bh][bw] blocks of 16 bytes, 16-byte aligned: written by encode, read by decode
    float*         out;              // decode: [H][W][3] f32
    uint32_t width, height, bw, bh;
    uint32_t rounds;                 // encode: least-squares rounds, 0 .. kBc6hMaxRounds
};

// ---- variance-guided lightmap finishing (mi_lightmap_finish_var; pt_kernels.hip "lmv_*") ----
// One pass of tracing.py lightmap_finish_var: lmv_init (the variance of the mean per texel from the bake's mean and second moments),
// lmv_blur (the colour weight's denominator per texel from the 3 x 3 blur of the variance) or lmv_atrous (one filter level of the image
// and its variance, step `step`, one kTile x kTile tile per block, the taps straight from HBM).  The mask and the dilation are
// lmf_mask's and lmf_dilate's.  Every pass reads `src` / `var_in` and writes `dst` / `var_out`: ping-pong, never in place.
struct LmvArgs {
    const float* src;                // [H][W][3] the previous pass's image (lmv_init: the raw bake)
    const float* m2;                 // [H][W][3] the bake's means of squares (lmv_init)
    const float* points;             // [H][W][3] guides (lmv_atrous)
    const float* normals;            // [H][W][3] guides: all-zero = empty texel
    const float* var_in;             // [H][W] the previous pass's variance (lmv_blur, lmv_atrous)
    const float* den;                // [H][W] lmv_blur's result (lmv_atrous)
    float*       dst;                // [H][W][3] (lmv_atrous)
    float*       var_out;            // [H][W] (lmv_init, lmv_atrous)
    float*       den_out;            // [H][W] (lmv_blur)
    uint32_t width, height, tiles_x, tiles_y;
    uint32_t step;                   // lmv_atrous: s = 2^level
    uint32_t npow;                   // normal_power_log2
    uint32_t samples;                // lmv_init without a counts plane: S
    float sigma_plane, reach, sigma_color, color_floor;
};

// ---- adaptive lightmap baking (mi_lightmap_select / _gather / _merge, mi_bake_lightmap_adaptive; pt_kernels.hip "lma_*") ----
// tracing.py lightmap_select as four passes: lmv_init with a counts plane (the variance of the mean per texel from the texel's own count,
// which mi_lightmap_finish_var_counts runs as well), lma_mark (the blur, the threshold, one flag per texel and the number
// of flags of each block of kLmaBlock consecutive texels), lma_scan (the exclusive prefix of the block counts, the total) and lma_fill
// (every block writes its texels' numbers at its offset, ascending).  lma_gather and lma_merge are lightmap_gather and lightmap_merge,
// one lane per slot / per list entry.  The list is the only value an address is made from, and every entry is tested against W * H first.
constexpr uint32_t kLmaBlock = 1024;             // texels per block of lma_mark / lma_fill (16 waves)
struct LmaArgs {
    const float*    image;           // [H][W][3] the bake's mean (lma_mark: the luminance)
    const float*    normals;         // [H][W][3] the centre table: all-zero = empty texel
    const float*    var;             // [H][W] lmv_init's result (lma_mark)
    float*          error;           // [H][W] or nullptr: sd (lma_mark)
    uint8_t*        flags;           // [H][W] 1 = selected (lma_mark writes, lma_fill reads)
    uint32_t*       block_counts;    // [blocks] (lma_mark writes, lma_scan reads)
    uint32_t*       block_offsets;   // [blocks] (lma_scan writes, lma_fill reads)
    uint32_t*       out_index;       // [capacity] (lma_fill)
    uint32_t*       out_count;       // [1] (lma_scan)
    uint32_t width, height, blocks, capacity;
    float target_rel, target_abs;
};
struct LmaListArgs {
    const uint32_t* index;           // [n] texel numbers; an entry >= width * height is skipped
    uint32_t n, width, height;
    // lma_gather
    const float*    points;          // [rows][H][W][3]
    const float*    normals;         // [rows][H][W][3]
    float*          out_points;      // [rows][slots][3]
    float*          out_normals;     // [rows][slots][3]
    uint32_t rows, slots;            // slots = ch * cw
    // lma_merge
    const float*    mean;            // [n][3] the round's mean, slot i for entry i
    const float*    m2_round;        // [n][3]
    float*          image;           // [H][W][3] in / out
    float*          m2;              // [H][W][3] in / out
    uint32_t*       counts;          // [H][W] in / out
    uint32_t round_samples;
};

// ---- irradiance volumes (mi_probe_volume_sample; pt_kernels.hip "pv_*") ----
// tracing.py probe_volume_sample: pv_prepare turns every probe's 27 SH coefficients into one 112-byte record (the coefficients times the
// cosine-lobe constants K_k, then the validity as 0.0 / 1.0: 28 floats, seven 16-byte loads), pv_sample interpolates the eight records
// around every point.  The grid constants are computed once on the host, in f32, as the helper does.
constexpr uint32_t kPvRecordFloats = 28;
constexpr uint32_t kPvMaxCount = 1024;           // per axis
constexpr uint32_t kPvMaxProbes = 1u << 22;      // 448 MiB of records
struct PvArgs {
    const float*   sh;               // [n_probes][9][3] (pv_prepare)
    const uint8_t* valid;            // [n_probes] or nullptr = all valid (pv_prepare)
    float*         records;          // [n_probes][28], 16-byte aligned: pv_prepare writes, pv_sample reads
    const float*   points;           // [n_points][3]
    const float*   normals;          // [n_points][3]: all-zero = empty texel
    float*         out_irradiance;   // [n_points][3]
    float*         out_weight;       // [n_points] or nullptr
    uint32_t n_probes, n_points;
    uint32_t counts[3];
    uint32_t normal_weight;          // MI_PV_NORMAL_WEIGHT
    float lo[3], cell[3], inv[3];    // cell_a = (hi_a - lo_a) / (float)n_a, inv_a = (float)n_a / (hi_a - lo_a)
};

}  // namespace pt
