/*
 * mi_rt.h — C ABI of the MI355X path-tracing hot path (libmi_rt.so).
 *
 * This header is the drop-in boundary for ONE path of mbk6/CS397RayTracingSP22:
 *     Scene::render_to_image()            src/util/tracing.rs:221-263
 *       -> Camera::generate_rays()        src/util/tracing.rs:159-209
 *       -> Scene::shade_ray()             src/util/tracing.rs:300-324
 *       -> Scene::intersect_ray()         src/util/tracing.rs:326-346
 *            -> {Sphere,Triangle,Plane,ConvexVolume,StaticMesh}::intersect_ray
 *                                         src/util/geometry.rs:300-321, 394-413, 430-450, 473-489, 501-526
 *            -> BVHNode / AABB / IndexedTriangle   src/util/geometry.rs:50-79, 93-119, 330-366
 *       -> Material::scatter()/emission() src/util/materials.rs:33-48, 56-71, 77-104, 113-149, 158-166
 *       -> Texture::sample()              src/util/texture.rs:26-32
 *
 * The reference has no FFI of its own (it is one Rust crate; the path is reached by
 * ordinary calls through `dyn Intersectable` / `dyn Material`).  What crosses this
 * boundary is therefore the *flattened* form of the reference's own structs: every
 * struct below mirrors one reference struct field for field, and `mi_scene_desc.objects`
 * keeps the order of `Scene.objects` (tracing.rs:215) because that order decides ties
 * (tracing.rs:335, strict `<`: the first object wins) and the order of RNG draws made by
 * ConvexVolume::intersect_ray (geometry.rs:517).
 *
 * Plain C: pointers, sizes, PODs.  No torch / HIP types in any signature; device
 * pointers and streams travel as `void*`.  Nothing unwinds across this boundary:
 * every entry point returns an mi_status and records a message for mi_last_error().
 *
 * Ownership: every input array is borrowed for the duration of the call only
 * (mi_scene_upload copies to the device).  Output buffers are allocated by the caller.
 * A mi_ctx owns its device memory; it is not re-entrant, distinct contexts may be
 * used from distinct threads.
 *
 * All arithmetic on the path is f32 (Vec3 = Vector3<f32>, tracing.rs:22).
 */
#ifndef MI_RT_H
#define MI_RT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_RT_ABI_VERSION 5

/* ---- status codes (reference: panics via assert!/expect/unwrap, geometry.rs:149-151) ---- */
typedef enum mi_status {
    MI_OK               =  0,
    MI_ERR_INVALID      = -1,  /* NULL pointer, bad index, bad size                      */
    MI_ERR_UNSUPPORTED  = -2,  /* reference feature outside the accelerated path         */
    MI_ERR_NO_DEVICE    = -3,  /* no gfx950 device / HIP runtime failure at create       */
    MI_ERR_HIP          = -4,  /* a HIP call failed (message holds hipGetErrorString)    */
    MI_ERR_OOM          = -5,
    MI_ERR_NO_SCENE     = -6   /* render called before a scene was uploaded              */
} mi_status;

/* ---- materials: `trait Material` implementors, materials.rs:20,51,74,107,152 ---- */
typedef enum mi_material_kind {
    MI_MAT_LAMBERTIAN    = 0,  /* Lambertian{albedo, emission}                      :20  */
    MI_MAT_METAL         = 1,  /* Metal{albedo, emission, roughness}                :51  */
    MI_MAT_DIELECTRIC    = 2,  /* Dielectric{idx_of_refraction}                     :74  */
    MI_MAT_PARAMETERIZED = 3,  /* ParameterizedMaterial{albedo,emission,rough,metal}:107 */
    MI_MAT_ISOTROPIC     = 4   /* Isotropic{albedo, emission}                       :152 */
} mi_material_kind;

typedef struct mi_material {
    int32_t kind;              /* mi_material_kind */
    float   albedo[3];
    float   emission[3];
    float   roughness;
    float   metallic;
    float   idx_of_refraction;
} mi_material;                 /* 40 bytes */

/* ---- primitives: `trait Intersectable` implementors, geometry.rs:389,424,468,495,127 ---- */
typedef enum mi_object_kind {
    MI_OBJ_SPHERE   = 0,       /* Sphere{center, radius, material}          geometry.rs:389 */
    MI_OBJ_TRIANGLE = 1,       /* Triangle{a, b, c, material}               geometry.rs:424 */
    MI_OBJ_PLANE    = 2,       /* Plane{point, normal, material}            geometry.rs:468 */
    MI_OBJ_VOLUME   = 3,       /* ConvexVolume{boundary, phase_function, density}      :495 */
    MI_OBJ_MESH     = 4,       /* StaticMesh                                geometry.rs:127 */
    MI_OBJ_SCENE    = 5        /* a nested Scene (`impl Intersectable for Scene`, tracing.rs:326) — only as the boundary of a ConvexVolume */
} mi_object_kind;

/* One entry of Scene.objects (tracing.rs:215), in the reference's order. */
typedef struct mi_object {
    int32_t kind;              /* mi_object_kind                         */
    int32_t index;             /* index into the typed array of that kind */
} mi_object;

typedef struct mi_sphere   { float center[3]; float radius; int32_t material; } mi_sphere;
typedef struct mi_triangle { float a[3]; float b[3]; float c[3]; int32_t material; } mi_triangle;
typedef struct mi_plane    { float point[3]; float normal[3]; int32_t material; } mi_plane;

/* ConvexVolume (geometry.rs:495-500).  `boundary` is `Arc<dyn Intersectable>` in the reference and its intersect_ray is called
 * twice per ray (geometry.rs:505,508: entry with t in [f32::MIN, f32::MAX], exit from t_entr + 1e-4).  boundary_kind says what it is:
 *   MI_OBJ_SPHERE (0, what every use in the reference is, tracing.rs:499-516): the sphere given INLINE by boundary_center / _radius;
 *   MI_OBJ_TRIANGLE, MI_OBJ_PLANE, MI_OBJ_MESH: entry boundary_index of the scene's typed array of that kind;
 *   MI_OBJ_SCENE: a nested Scene (its closest hit, first entry wins ties, tracing.rs:330-344) = the boundary_count entries of
 *                 mi_scene_desc.boundary_objects starting at boundary_index, each a Sphere / Triangle / Plane / StaticMesh.
 * The boundary object need not be listed in Scene.objects; its own material is ignored by the reference ("arbitrary",
 * tracing.rs:503).  A ConvexVolume or a Scene INSIDE a boundary is MI_ERR_UNSUPPORTED. */
typedef struct mi_volume {
    float   boundary_center[3];
    float   boundary_radius;
    float   density;
    int32_t phase_material;    /* index of the phase-function material (Isotropic) */
    int32_t boundary_kind;     /* mi_object_kind, 0 = the inline sphere */
    int32_t boundary_index;
    int32_t boundary_count;    /* MI_OBJ_SCENE only */
} mi_volume;

/* Texture (texture.rs:12-14) after `get_pixel(..).to_rgb()`: tightly packed RGB8,
 * row 0 = top row of the image file.  Decoding image files is load-time work outside
 * this path (texture.rs:16-25). */
typedef struct mi_texture {
    int32_t        width;
    int32_t        height;
    const uint8_t* rgb;        /* width*height*3 bytes */
} mi_texture;

/* StaticMesh (geometry.rs:127-134).  Geometry is tobj's single-index `Mesh`
 * (geometry.rs:140-148): one index per corner into positions/normals/texcoords.
 * normals and texcoords are required: the reference indexes them on every candidate
 * hit (geometry.rs:350,355) and would panic without them. */
typedef struct mi_mesh {
    const float*    positions;      /* n_vertices*3 */
    const float*    normals;        /* n_vertices*3 */
    const float*    texcoords;      /* n_vertices*2 */
    const uint32_t* indices;        /* n_triangles*3 */
    int32_t         n_vertices;
    int32_t         n_triangles;
    float           transform[16];      /* cgmath Matrix4, column-major     geometry.rs:132 */
    float           inv_transform[16];  /* transform.inverse_transform()    geometry.rs:168 */
    int32_t         material;           /* index, or -1 = material from textures (:255)     */
    int32_t         textures[5];        /* 0 albedo 1 emission 2 metallic 3 roughness 4 normal; -1 = None (:130) */
} mi_mesh;

typedef struct mi_scene_desc {
    const mi_object*   objects;    int32_t n_objects;
    const mi_sphere*   spheres;    int32_t n_spheres;
    const mi_triangle* triangles;  int32_t n_triangles;
    const mi_plane*    planes;     int32_t n_planes;
    const mi_volume*   volumes;    int32_t n_volumes;
    const mi_mesh*     meshes;     int32_t n_meshes;
    const mi_material* materials;  int32_t n_materials;
    const mi_texture*  textures;   int32_t n_textures;
    /* entries of the nested Scenes that serve as ConvexVolume boundaries (mi_volume.boundary_kind == MI_OBJ_SCENE); may be NULL / 0 */
    const mi_object*   boundary_objects;  int32_t n_boundary_objects;
    /* Scene.point_light_pos / Scene.ambient (tracing.rs:216-217): read by ShadingMode::Phong only */
    float              point_light_pos[3];
    float              ambient[3];
} mi_scene_desc;

/* ---- Camera (tracing.rs:138-155), field for field ---- */
#define MI_PROJ_ORTHOGRAPHIC 0    /* CameraProjectionMode::Orthographic (tracing.rs:196,200)           */
#define MI_PROJ_PERSPECTIVE  1
#define MI_SHADE_PHONG       0    /* ShadingMode::Phong, the debug shader (tracing.rs:277-297); own kernel, ignores `variant` */
#define MI_SHADE_PATHTRACE   1

typedef struct mi_camera_desc {
    float    eyepoint[3];
    float    view_dir[3];
    float    up[3];
    int32_t  projection_mode;
    int32_t  shading_mode;
    uint32_t path_depth;
    uint32_t path_samples;      /* 1 in every configuration (tracing.rs:370); != 1 runs MI_VARIANT_RECURSIVE */
    uint32_t screen_width;
    uint32_t screen_height;
    float    focal_length;
    float    focus_dist;
    float    lens_radius;
    uint32_t aa_sample_count;   /* perfect square (tracing.rs:152) */
    float    max_trace_dist;
    float    gamma;
} mi_camera_desc;

/* ---- render options (new: the reference RNG is unseeded thread_rng) ---- */
#define MI_TILE 32              /* image tiles are MI_TILE x MI_TILE pixels */

typedef struct mi_render_opts {
    uint32_t seed;              /* RNG stream key: (seed, y*W+x, sample)                 */
    int32_t  rank;              /* this process renders tiles t with t % world == rank   */
    int32_t  world;             /* number of ranks sharing the image (>=1)               */
    int32_t  variant;           /* 0 = default kernel; see mi_variant                    */
    int32_t  want_signature;    /* 1 = also produce per-pixel path signatures (diagnostic) */
    uint32_t flags;             /* MI_OPT_* bits, 0 = defaults                           */
    uint64_t max_state_bytes;   /* wavefront pipeline: upper bound on the HBM it may hold for path state and
                                 * sample slots (0 = what renders the frame in ONE batch, at most 60 % of the free HBM: a
                                 * whole 1080p / 256 spp frame is 110 GB).  A smaller budget means more, smaller sample
                                 * batches: same image, bit for bit, lower throughput (cfg2, round 4: one batch 72.7 ms;
                                 * 64 / 32 / 16 / 8 / 4 GB: +1 / +8 / +13 / +24 / +43 %: DESIGN.md section 4).
                                 * The smallest batch is one sample of every pixel of the rank (about 210 B per pixel, 280 B
                                 * with a two-stage mesh): a non-zero budget below that is MI_ERR_INVALID, never silently exceeded */
} mi_render_opts;               /* 32 bytes */

#define MI_OPT_NO_TILE_MASKS   1u   /* camera rays test every Scene.objects entry (no per-tile frustum masks): same image */
#define MI_OPT_REFERENCE_WALK  2u   /* meshes: walk the reference's own BVH (geometry.rs:94-119) node by node even where the
                                     * exact two-stage traversal would be used: same image, slower on large meshes */
#define MI_OPT_TWO_STAGE       4u   /* meshes: use the two-stage traversal for every mesh, whatever its size: same image */
#define MI_OPT_NO_LIST_TREE    8u   /* long lists: test every Triangle of Scene.objects one by one instead of walking the top-level tree the scene
                                     * compiler builds over them (>= 96 small triangles): same image */
#define MI_OPT_NO_FINAL_CULL   16u   /* path tracing without signatures: trace the final segment of every path like any other, even where no emitter
                                     * can be its closest hit (no final-segment cull): same image */
/* `flags` of mi_hemisphere_occlusion (below) */
#define MI_HEMI_WORLD_RADIUS 1u     /* t_max is a world-space radius: the interval of a sample ends at t_max / |d| */
/* mi_lightmap_texels / mi_bake_lightmap flags */
#define MI_LM_JITTER 1u             /* row r of a texel is a jittered position inside it, not its centre */
/* mi_probe_volume.flags (mi_probe_volume_sample, below) */
#define MI_PV_NORMAL_WEIGHT 1u      /* weight the eight corners by how far they lie in front of the surface */
/* `flags` of mi_lightmap_sample / mi_lightmap_sh_sample (below) */
#define MI_LS_NEAREST 1u            /* the reference's nearest-texel addressing (texture.rs:28-29), no interpolation */
/* `format` of mi_lightmap_pack / mi_lightmap_unpack / mi_lightmap_*_packed (below); 0 is reserved for f32 and refused there */
#define MI_LP_F16 1u                /* `channels` IEEE binary16 per texel, tightly packed (3 or 27 channels) */
#define MI_LP_RGB9E5 2u             /* one u32 per texel: three 9-bit mantissas and a shared 5-bit exponent (3 channels only) */
/* BC6H lightmaps (mi_lightmap_bc6h_*, mi_lightmap_sample_bc6h, below) */
#define MI_BC6H_BLOCK_BYTES 16u     /* one block ... */
#define MI_BC6H_BLOCK_DIM 4u        /* ... of 4 x 4 texels */
#define MI_BC6H_MODE 3u             /* the low five bits of the one block mode written and read */
#define MI_BC6H_MAX_ROUNDS 4u       /* mi_lightmap_bc6h_encode: the most least-squares rounds */

typedef enum mi_variant {
    MI_VARIANT_DEFAULT    = 0,  /* library picks (currently MI_VARIANT_WAVEFRONT)                  */
    MI_VARIANT_SIMPLE     = 1,  /* one segment per loop trip, mesh traversal in line (structural cross-check) */
    /* 2 was MI_VARIANT_PARKED: removed in ABI 3 (documented slower)            */
    MI_VARIANT_VOTED      = 3,  /* per-lane state machine; every BVH node step is a __ballot-voted phase */
    MI_VARIANT_VOTED_DIAG = 4,  /* VOTED + per-phase trip / active-lane counters (never timed)      */
    /* 5, 6 were MI_VARIANT_POOLED(_DIAG): removed in ABI 3                                          */
    MI_VARIANT_WAVEFRONT  = 7,  /* path state streamed through HBM, one kernel per phase (K1w); synchronises the stream */
    MI_VARIANT_RECURSIVE  = 8   /* shade_ray as written (tracing.rs:300-324), recursion on a per-lane stack: the only variant for
                                 * path_samples != 1 (chosen automatically); slow, bit-identical f32 image to the CPU restatement */
} mi_variant;

typedef struct mi_stats {
    uint64_t samples;           /* camera rays (paths) traced by this call                */
    uint64_t pixels;            /* pixels owned by this rank                              */
    uint32_t tiles;             /* tiles owned by this rank                               */
    uint32_t tiles_padded;      /* ceil(total_tiles/world): slots in the compact buffer   */
    float    kernel_ms;         /* path-tracing kernel, HIP events on the launch stream   */
    float    total_ms;          /* whole call incl. un-permute / tone-map / copies        */
    uint32_t scene_bytes;       /* bytes of scene data resident on device                 */
    uint32_t scene_in_lds;      /* 1 if the mesh BVH was staged into LDS                  */
} mi_stats;

typedef struct mi_ctx mi_ctx;

/* Create a context on HIP device `device` (one process per GPU: pass LOCAL_RANK). */
int  mi_ctx_create(int device, mi_ctx** out);
void mi_ctx_destroy(mi_ctx* ctx);

/* Flatten + upload a scene: replaces the construction of `Scene.objects`
 * (tracing.rs:374-540) and StaticMesh::build_bvh (geometry.rs:175-217; the BVH is
 * rebuilt here with the reference's topology). */
int  mi_scene_upload(mi_ctx* ctx, const mi_scene_desc* scene);

/* Replaces Scene::render_to_image (tracing.rs:221-263) for a whole image on one GPU.
 * out_rgb_f32: W*H*3 linear per-pixel means BEFORE saturation/gamma (parity surface), may be NULL.
 * out_rgb_u8 : W*H*3, the RgbImage byte layout of tracing.rs:226,254-256, may be NULL.
 * out_sig    : W*H u32 path signatures when opts->want_signature, may be NULL.
 * Host pointers. opts->rank/world must be 0/1. */
int  mi_render(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
               float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);

/* Multi-GPU building blocks; all pointers are DEVICE pointers on ctx's device and
 * `stream` is a hipStream_t (NULL = default stream).  Work is queued on `stream`; the
 * megakernel variants never synchronise, the default wavefront variant drives its per-segment
 * iterations from the host and synchronises `stream` inside mi_render_tiles_device.
 *
 * mi_render_tiles_device: rank `opts->rank` of `opts->world` renders its tiles
 *   (tile t -> rank t % world, slot t / world; tiles are numbered row-major over a grid whose row length is the image's tile
 *   columns rounded up to the next integer coprime with `world`, so that every rank meets every column class — the surplus
 *   columns hold no pixel and are written as zeros; mi_compact_size gives the counts) into a compact tile-major buffer
 *   d_compact[tiles_padded][MI_TILE*MI_TILE][3] f32 (row-major inside a tile; pixels
 *   outside the image are written as 0).  d_sig (may be NULL) is [tiles_padded][MI_TILE*MI_TILE] u32.
 * mi_unpermute_device: gathered buffer [world][tiles_padded][1024][3] -> row-major W*H*3 f32.
 * mi_tonemap_device: tracing.rs:244-256 (saturate toward white, gamma, quantise) -> W*H*3 u8. */
int  mi_compact_size(const mi_camera_desc* cam, int32_t world, uint32_t* tiles_total, uint32_t* tiles_padded);
int  mi_render_tiles_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                            void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);
/* Progressive / resumable accumulation (the reference renders all `aa_sample_count` samples of a
 * pixel in one go, tracing.rs:233-241; this splits that loop without changing its result).
 * Traces samples [sample_begin, sample_end) of every pixel of this rank and adds them IN ORDER to the
 * caller-held accumulator d_accum_f32x4[tiles_padded*MI_TILE*MI_TILE] (float4: xyz = running sums,
 * w = bits of the running signature sum).  sample_begin == 0 starts the sums from zero (the buffer
 * need not be cleared).  When sample_end == aa_sample_count the per-pixel means (and signatures) are
 * written to d_compact_f32 / d_sig_u32 exactly as mi_render_tiles_device does; otherwise both may be
 * NULL.  Calls must cover [0, aa_sample_count) in increasing, gap-free order; the accumulator may be
 * copied out and back in between (checkpoint / resume, also into another context with the same
 * scene, camera, seed, rank and world).  The final image is bit-identical to a one-call render.
 * Default (wavefront) path-tracing variant only. */
int  mi_render_samples_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                              uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                              void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);
int  mi_unpermute_device(mi_ctx* ctx, const mi_camera_desc* cam, int32_t world,
                         const void* d_gathered_f32, void* d_image_f32, void* stream);
int  mi_tonemap_device(mi_ctx* ctx, const mi_camera_desc* cam,
                       const void* d_image_f32, void* d_image_u8, void* stream);

/* Elapsed time of the most recent path-tracing or ray-query kernel of this ctx (HIP events on its
 * launch stream); synchronises on the stop event. */
int  mi_last_kernel_ms(mi_ctx* ctx, float* ms);

/* ---- ray queries: the reference's two calls that take a ray of the CALLER's making (added within ABI version 5: the version number
 * is unchanged, a caller that may meet an older library detects these four by symbol lookup) ----
 * mi_intersect_rays: `impl Intersectable for Scene`, Scene::intersect_ray (tracing.rs:326-346), for n_rays rays: the closest hit over
 *   Scene.objects in [t_min, t_max], the first object winning a tie.  Picking, visibility and occlusion probes, light baking, cameras
 *   the reference does not have.  t_max = +infinity is legal; a NaN t_min or t_max is MI_ERR_INVALID.
 * mi_shade_rays: Scene::shade_ray (tracing.rs:300-324) at level 0 for n_rays rays, as written (the recursive estimator of
 *   MI_VARIANT_RECURSIVE, bit-identical to the CPU restatement for every path_samples; not a tuned path).  `cam` supplies path_depth,
 *   path_samples and max_trace_dist; its screen_* fields and aa_sample_count are ignored.  shading_mode Phong and path_depth > 64 are
 *   MI_ERR_UNSUPPORTED.  path_samples == 0 (tracing.rs:318 divides by it) and a NaN max_trace_dist are MI_ERR_INVALID, as in mi_render.
 * Directions are used as given, NOT normalised (the reference does not normalise them either: distances are in units of |dir|).
 * Ray i draws from the RNG stream (seed, pixel = first_key + i, sample = 0), fresh: no Camera::generate_rays draws come first.  Only
 * ConvexVolume::intersect_ray and the scatters read it.  A batch split over several calls with first_key advanced by the rays already
 * done gives the answers of one call.  Non-finite origins or directions are not rejected: a "hit" at a NaN distance is kept
 * in the kernels' kind-grouped order, not in Scene.objects order (the deviation DESIGN.md section 2 (v) records; finite rays are exact).
 * The plain forms take HOST pointers and block: they upload, run and download in chunks through a buffer of their own, so device
 * scratch stays bounded whatever n_rays is.  The _device forms take DEVICE pointers on ctx's device and queue one kernel on `stream`
 * (a hipStream_t, NULL = default stream) without synchronising.  Neither touches the buffers mi_reserve sized.
 * n_rays == 0 is MI_OK and launches nothing.  mi_last_kernel_ms afterwards gives the query kernel's time (the sum over the chunks of a
 * host-pointer call).
 * Outputs of mi_intersect_rays (each [n_rays] records; every one except out_object may be NULL, and when all of out_hitpoint ..
 * out_material are NULL the visibility form of the kernel runs, which never fetches shading data):
 *   out_object   int32            index into Scene.objects, -1 = None (REQUIRED); for a miss every other output holds zeros
 *   out_distance float            RayHit.distance (object-space t for a StaticMesh, geometry.rs:304-305)
 *   out_hitpoint float[3]         RayHit.hitpoint (world space)
 *   out_normal   float[3]         RayHit.normal, facing the ray (zero inside a ConvexVolume, geometry.rs:520)
 *   out_flags    int32            bit 0 = frontface, bit 1 = has_tex_coords (StaticMesh hits)
 *   out_uv       float[2]         RayHit.tex_coords (geometry.rs:356)
 *   out_material mi_material      the material at the hit (StaticMesh::get_material_at_uv for meshes, the phase function for a volume) */
int  mi_intersect_rays(mi_ctx* ctx, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                       uint32_t seed, uint32_t first_key, int32_t* out_object, float* out_distance, float* out_hitpoint,
                       float* out_normal, int32_t* out_flags, float* out_uv, mi_material* out_material);
int  mi_intersect_rays_device(mi_ctx* ctx, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                              uint32_t seed, uint32_t first_key, int32_t* out_object, float* out_distance, float* out_hitpoint,
                              float* out_normal, int32_t* out_flags, float* out_uv, mi_material* out_material, void* stream);
int  mi_shade_rays(mi_ctx* ctx, const mi_camera_desc* cam, uint32_t n_rays, const float* origins, const float* dirs,
                   uint32_t seed, uint32_t first_key, float* out_rgb);
int  mi_shade_rays_device(mi_ctx* ctx, const mi_camera_desc* cam, uint32_t n_rays, const float* origins, const float* dirs,
                          uint32_t seed, uint32_t first_key, float* out_rgb, void* stream);

/* ---- occlusion queries: "is anything in the way?" (added within ABI version 5 like the four above: detect by symbol lookup) ----
 * mi_occluded_rays: out_occluded[i] = 1 exactly when Scene::intersect_ray(ray_i, t_min, t_max_i) (tracing.rs:326-346) returns Some,
 *   that is when some entry of Scene.objects returns Some from its own intersect_ray over that interval; 0 otherwise.  The same answer
 *   as `mi_intersect_rays(...).out_object >= 0`, but a ray is done at its first accepted hit (any-hit: shadow rays, visibility between
 *   points, ambient occlusion, baking).  Exact, not approximate: `best_hit` never goes back to None, so the answer is the OR over the
 *   objects in any order — also for non-finite rays.
 * ray_t_max: NULL, then every ray uses t_max; or [n_rays] floats that REPLACE t_max ray by ray (t_max is then ignored apart from its
 *   NaN check).  +infinity is legal.  The host form refuses a NaN t_min / t_max and a NaN anywhere in ray_t_max with MI_ERR_INVALID.
 *   The _device form checks only the scalars: a NaN entry of a device ray_t_max gives an UNSPECIFIED answer for that ray (0 or 1) and
 *   never faults or disturbs another ray.
 * Directions are used as given, NOT normalised, and the interval is in units of |dir|: the segment from a to b is
 *   origin = a, dir = b - a, [t_min, t_max] = [eps, 1 - eps]; a unit direction towards a light at distance L takes ray_t_max = L - eps.
 * Ray i draws from the RNG stream (seed, first_key + i, 0) as in mi_intersect_rays (only a ConvexVolume reads it), so a batch may be
 *   split over calls with first_key advanced.  out_occluded: [n_rays] bytes, 0 or 1 (REQUIRED).
 * Host / _device forms, chunking, n_rays == 0, the buffers of mi_reserve and mi_last_kernel_ms: as for mi_intersect_rays.  NULL origins,
 *   dirs or out_occluded are MI_ERR_INVALID, a context without a scene is MI_ERR_NO_SCENE. */
int  mi_occluded_rays(mi_ctx* ctx, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                      const float* ray_t_max, uint32_t seed, uint32_t first_key, uint8_t* out_occluded);
int  mi_occluded_rays_device(mi_ctx* ctx, uint32_t n_rays, const float* origins, const float* dirs, float t_min, float t_max,
                             const float* ray_t_max, uint32_t seed, uint32_t first_key, uint8_t* out_occluded, void* stream);

/* ---- hemisphere occlusion: ambient-occlusion baking with rays made ON THE GPU (added within ABI version 5 like the queries above:
 * detect by symbol lookup) ----
 * For each of n_points surface points the kernel draws n_samples hemisphere directions about the point's normal, asks the any-hit
 *   question of mi_occluded_rays for each and reduces per point: nothing per ray crosses the bus.  `points` and `normals` are
 *   [n_points][3] f32.
 * Sample s of point i, s = first_sample + k the GLOBAL sample index, k < n_samples:
 *   direction d = exactly what Lambertian::scatter -> sample_hemisphere (materials.rs:33-48, 171-178) returns for a hit whose normal is
 *     normals[i] — the normal as given, NOT normalised — drawn from a fresh RNG stream (seed, first_key + i, 2s).  d is NOT normalised:
 *     rand_sphere_vec returns a point of the unit ball, |d| <= 1.
 *   ray: origin = points[i] as given (the caller applies any offset), direction d, interval [t_min, t_max] in units of |d| as everywhere
 *     in this ABI, tested as by mi_occluded_rays — Scene::intersect_ray(..).is_some() — with a second fresh stream
 *     (seed, first_key + i, 2s + 1), which only a ConvexVolume reads.  Two streams, so that the free-flight draw is independent of the
 *     direction.
 * flags: 0, or MI_HEMI_WORLD_RADIUS (defined with the MI_OPT_ bits above): the upper end of the interval becomes t_max / sqrtf(dot(d, d)), in f32 with IEEE `/` and sqrtf,
 *   which makes t_max a world-space radius; t_min is left alone.  Any other bit is MI_ERR_INVALID.
 * out_open[i] (REQUIRED, uint32): how many of the n_samples samples are NOT occluded.  out_bent[i] (float[3], may be NULL): the f32 sum
 *   of d over those samples, taken in a fixed order that depends only on (first_sample, n_samples): two identical calls give identical
 *   bits (no float atomics).  Divide by out_open[i] and normalise for the bent normal.
 * Splitting a bake: by points (first_key advanced by the points already done) and by samples (first_sample advanced by the samples
 *   already done, the counts added up) both give the counts of one call EXACTLY, because every sample has streams of its own.  The bent
 *   sums of a split by samples add up to the one call's within f32 rounding, not bit for bit.
 * n_points == 0 is MI_OK and launches nothing.  MI_ERR_INVALID: n_samples == 0 or > 65535, first_sample + n_samples > 2^31, NULL points,
 *   normals or out_open, a NaN t_min or t_max.  A context without a scene is MI_ERR_NO_SCENE.  A zero or non-finite normal or point gives
 *   an UNSPECIFIED count (and bent sum) for that point; it never faults and never disturbs another point.
 * Host / _device forms, the buffers of mi_reserve and mi_last_kernel_ms: as for mi_occluded_rays.  The host form chunks over points so
 *   that one launch holds at most about 2^24 rays. */
int  mi_hemisphere_occlusion(mi_ctx* ctx, uint32_t n_points, const float* points, const float* normals, uint32_t first_sample,
                             uint32_t n_samples, float t_min, float t_max, uint32_t flags, uint32_t seed, uint32_t first_key,
                             uint32_t* out_open, float* out_bent);
int  mi_hemisphere_occlusion_device(mi_ctx* ctx, uint32_t n_points, const float* points, const float* normals, uint32_t first_sample,
                                    uint32_t n_samples, float t_min, float t_max, uint32_t flags, uint32_t seed, uint32_t first_key,
                                    uint32_t* out_open, float* out_bent, void* stream);

/* ---- ray-table rendering: a whole render from rays of the CALLER's making, through the wavefront pipeline (added within ABI version 5
 * like the queries above: detect by symbol lookup) ----
 * A ray table replaces Camera::generate_rays (tracing.rs:159-209) for one render; the rest of Scene::render_to_image (tracing.rs:221-263)
 *   stays: per-pixel sums in sample order, the mean, saturation / gamma / bytes.  Fisheye, panoramic and stereo cameras, light probes,
 *   lightmap baking at any sample count: the tuned path of mi_render (classes, LDS walkers, two-stage traversal, batches), not the
 *   recursive kernel of mi_shade_rays.  (A lightmap whose rays are hemisphere samples about a normal needs no ray table at all:
 *   mi_render_points below takes the points and normals and draws the directions on the GPU.)
 * Layout: the image is cam->screen_width x screen_height (W x H) with cam->aa_sample_count samples per pixel.  `origins` and `dirs` are
 *   two arrays [rays_per_pixel][H][W][3] f32: ray (s, y, x) sits at ((s*H + y)*W + x)*3 (indexed in 64 bits).  rays_per_pixel is
 *   aa_sample_count (sample s of a pixel uses row s) or 1 (every sample of a pixel uses the same ray); anything else is MI_ERR_INVALID.
 * RNG: sample s of pixel (x, y) draws from the stream (seed, y*W + x, s), fresh: no Camera::generate_rays draws come first.  That is
 *   mi_shade_rays with first_key = 0 for s = 0.  Only ConvexVolume::intersect_ray and the scatters read the stream.
 * Rays: directions are used as given, NOT normalised; t_min = 0.001, t_max = cam->max_trace_dist, as in mi_render.  Non-finite rays are
 *   not rejected and never fault; their results follow DESIGN.md section 2 (v), as for mi_intersect_rays (finite rays are exact).
 * Camera fields read: screen_width, screen_height, aa_sample_count (any value in 1 .. 65535: it need NOT be a perfect square, the
 *   square exists for generate_rays' jitter grid only), path_depth, path_samples, shading_mode, max_trace_dist, gamma.  eyepoint,
 *   view_dir, up, projection_mode, focal_length, focus_dist and lens_radius are IGNORED and may hold anything, non-finite values included.
 * Refusals (each with a message, nothing is launched): path_samples != 1 or MI_SHADE_PHONG, and a variant other than DEFAULT /
 *   WAVEFRONT, are MI_ERR_UNSUPPORTED (mi_shade_rays is the call for path_samples != 1); path_samples == 0, a NaN max_trace_dist, a bad
 *   gamma, a bad image size, aa_sample_count == 0 and NULL tables are MI_ERR_INVALID; a context without a scene is MI_ERR_NO_SCENE.
 * Masks: the primary-ray tile masks and dead-tile culling are derived from the camera, so they are OFF for these calls whatever
 *   opts->flags says (the effect of MI_OPT_NO_TILE_MASKS; entry 7 of mi_last_pipeline_counts is 0).  The other MI_OPT_* keep their meaning.
 * Output: sample order, the mean, the f32 / u8 / signature outputs and the compact tile-major layout are those of mi_render /
 *   mi_render_tiles_device.  mi_reserve, max_state_bytes, mi_last_kernel_ms and mi_last_pipeline_ms / _counts behave as for mi_render.
 * mi_render_rays: HOST pointers, blocking, opts->rank / world must be 0 / 1.  The table is uploaded into a buffer the context owns
 *   (grown on demand, freed with the context; never the buffers mi_reserve sized nor the queries' chunk buffer; MI_ERR_OOM if it cannot
 *   be allocated), then: render, un-permute, tone-map, download, as mi_render.
 * mi_render_rays_device: DEVICE pointers on ctx's device; mi_render_tiles_device and mi_render_samples_device in one call.  Rank
 *   opts->rank of opts->world renders its tiles into the compact buffer.  [sample_begin, sample_end) = [0, aa_sample_count) with
 *   d_accum_f32x4 == NULL is a whole render; any other range follows mi_render_samples_device's rules (accumulator required, calls
 *   cover the range in order, outputs written by the call that ends at aa_sample_count).  The table must stay valid until the call
 *   returns (it synchronises `stream`).  mi_multi_* takes no table. */
int  mi_render_rays(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                    const float* origins, const float* dirs, uint32_t rays_per_pixel,
                    float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);
int  mi_render_rays_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                           const float* d_origins, const float* d_dirs, uint32_t rays_per_pixel,
                           uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                           void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);

/* ---- point-table rendering: lightmap / irradiance baking with the rays made on the GPU (added within ABI version 5: detect by symbol
 * lookup) ----
 * mi_render_rays for a table of SURFACE POINTS and NORMALS: 24 B per texel cross the bus whatever the sample count, and the camera pass
 *   draws the direction of every sample itself.  The pixel's value is the mean over its aa_sample_count samples of
 *   Scene::shade_ray(Ray(p, d_s), 0) (tracing.rs:300-324) with d_s = sample_hemisphere(n) (materials.rs:171-178), the direction a
 *   Lambertian::scatter (materials.rs:33-48) would take at that point: the incoming radiance a Lambertian texel gathers, cosine-weighted
 *   by the sampling — what a lightmap or an irradiance bake stores (multiply by the albedo for outgoing radiance).
 * Layout: `points` and `normals` are two arrays [rows_per_pixel][H][W][3] f32, texel (row, y, x) at ((row*H + y)*W + x)*3 (indexed in 64
 *   bits); rows_per_pixel is aa_sample_count (sample s uses row s: a jittered position inside the texel) or 1 (every sample of the pixel
 *   starts at the same point); anything else is MI_ERR_INVALID.
 * Two streams per sample s of pixel (x, y):
 *   direction: (seed, W*H + y*W + x, s), fresh: rand_sphere_vec, y = |y|, rotate_from_unit_y(n, .) — sample_hemisphere with the normal as
 *     given (NOT normalised: only its direction matters to the rotation, whose quaternion is normalised) and the direction not normalised
 *     either (|d| <= 1: a point of the unit ball).  Pixel keys >= W*H are used by no path stream of the image; W, H <= 32768 keeps the
 *     key below 2^31.
 *   path: (seed, y*W + x, s), fresh: the stream of mi_render_rays.
 *   Hence the equivalence: mi_render_points(points, normals) == mi_render_rays(points, d) for the table d of those directions, the same
 *   f32 operations in the same order.
 * Empty texels: a normal whose three components are all zero (either sign of zero) marks a texel no surface covers.  It draws nothing
 *   and traces nothing; its samples are zero: f32 0, u8 tone-mapped 0, signature 0.  An image of empty texels only is MI_OK and black.
 * Origin: the point is used as given.  The caller applies any offset along the normal (lightmap_texels' `offset` in Python); t_min = 0.001
 *   and t_max = cam->max_trace_dist are in units of |d| <= 1, not of world length, as for any unnormalised ray.
 * Non-finite input: a NaN or infinite point or normal is not rejected and never faults; it gives an unspecified value for that pixel
 *   only (no address depends on the table's values; every other pixel's bits are those of the clean render).
 * Everything else is mi_render_rays', word for word: the camera fields read and ignored, the refusals (NULL tables, rows_per_pixel,
 *   path_samples != 1, MI_SHADE_PHONG, a variant other than DEFAULT / WAVEFRONT, no scene, rank / world), masks OFF (entry 7 of
 *   mi_last_pipeline_counts is 0), mi_reserve, max_state_bytes, mi_last_kernel_ms, mi_last_pipeline_ms / _counts, the output layouts.
 *   stats->samples counts slots, W*H*aa_sample_count for a whole image, empty texels included (the device form cannot know the table's
 *   contents without reading it).
 * mi_render_points: HOST pointers, blocking, rank / world 0 / 1; the tables are uploaded into the context's table buffer (mi_render_rays').
 * mi_render_points_device: DEVICE pointers; the sample range, the accumulator and the rank / world rules are mi_render_rays_device's.
 *   mi_multi_* takes no table. */
int  mi_render_points(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                      const float* points, const float* normals, uint32_t rows_per_pixel,
                      float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);
int  mi_render_points_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                             const float* d_points, const float* d_normals, uint32_t rows_per_pixel,
                             uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4,
                             void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);

/* ---- lightmap atlas: the point table of a mesh's uv atlas made on the GPU (added within ABI version 5: detect by symbol lookup) ----
 * The table mi_render_points reads, rasterised from a single-index triangle mesh in HBM: `out_points` and `out_normals`
 *   [rows][H][W][3] f32 and, when not NULL, `out_triangle` [rows][H][W] int32 (the winning triangle's index, -1 = empty texel).  Of the
 *   mi_mesh it reads positions, normals, texcoords, indices, the two counts and transform; inv_transform, material and textures are
 *   ignored.  No scene is needed.  These are the semantics of lightmap_texels (Python), from "texel centre" to "sample position":
 * Sample position: row r of texel (x, y) lies at u = (x + jx) / W, v = 1 - (y + jy) / H, in f64 — the inverse of Texture::sample's
 *   x = floor(u W), y = floor((1 - v) H) (texture.rs:28-29).  Without MI_LM_JITTER jx = jy = 0.5, the texel's centre, and every row
 *   is the same row.  With MI_LM_JITTER jx, then jy, are the first two gen_range(0.0..1.0) draws (f32, promoted to f64) of the fresh stream
 *   (seed, 2*W*H + y*W + x, r).  Keys in [2 W H, 3 W H) are used by no other stream of the image (paths: [0, W H), directions:
 *   [W H, 2 W H)); 3*W*H > 2^31 is MI_ERR_INVALID, with or without the flag.
 * Coverage: a triangle (a, b, c) whose uv area is finite and not zero covers the sample when its three edge functions
 *   ea = ((ub - u)(vc - v) - (vb - v)(uc - u)) * sign(area), eb, ec (cyclic) are >= 0, evaluated in f64 without fused multiply-adds.
 *   Where several triangles cover a sample the LOWEST triangle index wins.  NaN texcoords cover nothing; a triangle with an index
 *   >= n_vertices covers nothing (device form; its vertices are not read).
 * Resolve: weights ea / (ea + eb + ec), ...; position and normal interpolated in f64; the position through transform, the normal through
 *   the inverse transpose of its upper 3 x 3 (computed in f64 from transform), normalised; point += offset * normal; one rounding to
 *   f32.  A sample nothing covers, and one whose normal has no or no finite length, is all zero with triangle -1: the empty-texel mark
 *   of mi_render_points.  The result does not depend on scheduling: the winner is an integer minimum, nothing is summed across threads.
 * rows: 1 .. 65535.  A mesh of 0 triangles is MI_OK and all empty.  MI_ERR_INVALID (each with a message, checked before the context):
 *   NULL mesh, arrays or outputs (out_triangle may be NULL), width or height of 0 or above 32768, rows of 0 or above 65535, an unknown
 *   flag, a NaN offset, and, host forms only, an index >= n_vertices.
 * Scratch: per call 16 B per 32 x 32-texel tile plus 4 B per (triangle, tile) pair of the triangles' uv boxes, in buffers the context
 *   owns (grown on demand, freed with the context, never the buffers mi_reserve sized; MI_ERR_OOM if they cannot be allocated).  The
 *   pairs are bounded by n_triangles * tiles and capped at 2^30; tiles whose pairs do not fit test the whole mesh: slower, same result.
 * mi_lightmap_texels: HOST pointers, blocking; mesh and outputs pass through buffers the context owns.
 * mi_lightmap_texels_device: the mesh's four arrays and the outputs are DEVICE pointers on ctx's device.  Queues on `stream` and does
 *   not synchronise, except when it has to grow its scratch; it sizes the pair list by what the previous call needed.
 *   mi_last_kernel_ms reports the kernels of the last call.
 * mi_bake_lightmap: the whole bake, blocking: W x H = cam->screen_width x screen_height, seed = opts->seed, rows = aa_sample_count with
 *   MI_LM_JITTER, else 1.  Uploads the mesh, makes the table in the context's table buffer (the one mi_render_rays uploads into), then
 *   does exactly what mi_render_points does from there: the same image, bit for bit, as mi_render_points on the table
 *   mi_lightmap_texels returns.  Every refusal and camera rule of mi_render_points applies, word for word, and every refusal above;
 *   out_triangle ([rows][H][W]) may be NULL.  Only the mesh crosses the bus. */
int  mi_lightmap_texels(mi_ctx* ctx, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags,
                        uint32_t seed, float offset, float* out_points, float* out_normals, int32_t* out_triangle);
int  mi_lightmap_texels_device(mi_ctx* ctx, const mi_mesh* mesh, uint32_t width, uint32_t height, uint32_t rows, uint32_t flags,
                               uint32_t seed, float offset, float* out_points, float* out_normals, int32_t* out_triangle, void* stream);
int  mi_bake_lightmap(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                      float offset, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, int32_t* out_triangle, mi_stats* stats);

/* ---- lightmap finishing: edge-aware a-trous filter and gutter dilation (added within ABI version 5: detect by symbol lookup) ----
 * Turns the raw per-texel mean of a bake (mi_bake_lightmap's out_rgb_f32: empty texels exactly zero) into an image a renderer can sample:
 *   a denoise guided by the atlas's own world-space point and normal per texel, which cannot leak light between charts that are
 *   neighbours in uv only, then edge padding, so that bilinear filtering and mip-mapping do not smear black onto the surface at uv seams.
 *   These are the semantics of lightmap_finish (Python), which is the definition; the result equals the helper's BIT FOR BIT: pure f32,
 *   every operation one of + - * /, fabsf, fmaxf, comparisons and exact int-to-float conversions, in the order written here, no fused
 *   multiply-add, IEEE division.  No scene is needed.
 * Layout: `image`, `points`, `normals` and `out_image` are [H][W][3] f32, out_valid [H][W] bytes (0 / 1; may be NULL).  The guides are the
 *   CENTRE table (mi_lightmap_texels with rows = 1 and no MI_LM_JITTER), also for a jittered bake.  A texel is covered when its guide
 *   normal is not all-zero (either sign of zero), the empty-texel mark of mi_render_points; normals and points are used as given.
 * Filter: levels i = 0 .. levels-1 with step s = 2^i, each reading the previous level's image (ping-pong, never in place).  For a covered
 *   texel p the 25 taps q = p + s (dx, dy), dy outer -2 .. 2, dx inner -2 .. 2; a tap outside the image or on an empty texel is skipped.
 *   With D = P_q - P_p:
 *     h  = H5[dy+2] * H5[dx+2], H5 = { 1/16, 1/4, 3/8, 1/4, 1/16 }
 *     wn = fmaxf(0, (n_p.x n_q.x + n_p.y n_q.y) + n_p.z n_q.z), then wn = wn * wn repeated normal_power_log2 times
 *     wp = fmaxf(0, 1 - fabsf((n_p.x D.x + n_p.y D.y) + n_p.z D.z) / sigma_plane)
 *     reach: the tap is accepted only when (D.x D.x + D.y D.y) + D.z D.z <= (r r) (float)(dx dx + dy dy), r = reach * (float)s: `reach`
 *       is the world length one texel step may span, a hard cut against taps that land in another chart.  The centre tap is accepted
 *       without the comparison (0 <= 0 for a finite reach; taken literally an infinite reach would make its bound inf * 0).
 *     wc = fmaxf(0, 1 - ((|dr| + |dg|) + |db|) / (sigma_color / (float)s)), the differences between the current level's colours at q and p
 *     w  = ((h wn) wp) wc;  sw = sw + w;  sc[k] = sc[k] + w c_q[k]
 *   and the texel becomes sc / sw.  Empty texels are +0.0 at every level.  +inf for sigma_plane, reach or sigma_color turns that
 *   weight off (1 - x / inf == 1 for finite x).
 * Dilation: `dilate` passes after the filter, ping-pong again; valid starts as covered.  In one pass a texel that is not valid and has a
 *   valid 8-neighbour in the PREVIOUS pass's state takes the f32 sum of those neighbours' colours — dy outer -1 .. 1, dx inner -1 .. 1,
 *   without the centre, added in that order from +0.0 — divided by (float)count, and is valid from the next pass on.  Valid texels never
 *   change.  A texel turns valid in the pass that equals its Chebyshev distance from the nearest covered texel.
 * levels == 0 && dilate == 0 copies covered texels and zeroes empty ones.  An all-empty table is MI_OK: a zero image, out_valid all 0.
 * Non-finite image or guide values are not rejected and never fault; they give unspecified values only for texels whose footprint
 *   (Chebyshev radius 2 (2^levels - 1) + dilate) reaches them; every other texel keeps the bits of the clean run.  No address depends on
 *   a table value.  The result does not depend on scheduling: no atomics, nothing is summed across threads.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): NULL image, points, normals or out_image; width
 *   or height of 0 or above 32768; levels > 8, normal_power_log2 > 7, dilate > 256; a sigma_plane, reach or sigma_color that is NaN or <= 0.
 * Scratch: two [H][W][3] f32 images and two [H][W] byte masks in a buffer the context owns (grown on demand, freed with the context,
 *   never the buffers mi_reserve sized; MI_ERR_OOM if it cannot be allocated).  One kernel per level and per pass (a level stages its
 *   32 x 32 tile and halo in LDS for small steps and reads HBM directly for large ones: the same bits); mi_last_kernel_ms reports
 *   their sum.
 * mi_lightmap_finish: HOST pointers, blocking; the tables pass through a buffer the context owns; out_image may alias image.
 * mi_lightmap_finish_device: DEVICE pointers on ctx's device.  Queues on `stream` and does not synchronise, except when it has to grow
 *   its scratch.  An out_image that overlaps image, points or normals is MI_ERR_INVALID. */
int  mi_lightmap_finish(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* points, const float* normals,
                        uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                        uint32_t dilate, float* out_image, uint8_t* out_valid);
int  mi_lightmap_finish_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* points, const float* normals,
                               uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                               uint32_t dilate, float* out_image, uint8_t* out_valid, void* stream);

/* ---- lightmap variance: second moments of a point-table bake (added within ABI version 5: detect by symbol lookup) ----
 * mi_render_points / mi_bake_lightmap with a second output: per texel and colour channel the MEAN OF THE SQUARES of its aa_sample_count
 *   samples, beside their mean.  Together the two give each texel's own noise (mi_lightmap_finish_var below turns them into the variance
 *   of the mean), which a filter, or a caller who decides where more samples are worth their time, needs and the mean alone cannot give.
 * Definition: out_m2 is [H][W][3] f32, m2_c = (sum_s L_s.c * L_s.c) / (float)S, S = aa_sample_count, L_s the sample the mean is made of.
 *   Each of the three sums is accumulated in f32 in sample order from +0.0 (one multiply and one add per sample, not fused) and divided
 *   once at the end by (float)S, the division the mean uses: out_m2 is bit-identical across max_state_bytes, ranks, MI_OPT_* flags and
 *   progressive splits.  With S == 1, m2_c == mean_c * mean_c exactly.  Empty texels (an all-zero normal) are +0.0.
 * Plain outputs: the mean (f32), u8 and signature outputs are mi_render_points' / mi_bake_lightmap's BIT FOR BIT: the sums of squares
 *   are a further reduction (wf_reduce_m2) of the same sample slots behind wf_reduce in every batch; no other kernel runs differently.
 * Everything else is mi_render_points' / mi_bake_lightmap's, word for word: the tables, the two streams, the camera fields read and
 *   ignored, the refusals (NULL tables, rows_per_pixel, path_samples != 1, MI_SHADE_PHONG, a variant other than DEFAULT / WAVEFRONT, no
 *   scene, rank / world, the mesh's), masks OFF, mi_reserve, max_state_bytes, stats->samples = W*H*aa_sample_count.  Entry 7 of
 *   mi_last_pipeline_ms is the time of wf_reduce_m2 after these calls.
 * mi_render_points_moments: HOST pointers, blocking, rank / world 0 / 1; out_m2 is required (MI_ERR_INVALID if NULL, checked first), the
 *   other outputs may be NULL.  The compact records and the un-permuted plane live in a buffer the context owns (grown on demand, freed
 *   with the context, never the buffers mi_reserve sized; MI_ERR_OOM if it cannot be allocated).
 * mi_render_points_moments_device: DEVICE pointers; the sample range, the accumulator and the rank / world rules are
 *   mi_render_rays_device's.  d_compact_m2 is [tiles_padded][1024][3] f32 in the compact tile-major layout (mi_unpermute_device turns it
 *   into [H][W][3]), output AND running accumulator: the call with sample_begin == 0 starts the sums from zero (the buffer need not be
 *   cleared), later calls add to it, the call that ends at aa_sample_count divides; it may be copied out and back between calls.  Slots
 *   outside the image and padding slots are written as zeros by every call.  d_compact_m2 == NULL is legal and is then exactly
 *   mi_render_points_device.  mi_multi_* takes no table.
 * mi_bake_lightmap_moments: mi_bake_lightmap with out_m2 (required): the same moments, bit for bit, as mi_render_points_moments on the
 *   table mi_lightmap_texels returns. */
int  mi_render_points_moments(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                              const float* points, const float* normals, uint32_t rows_per_pixel, float* out_m2,
                              float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);
int  mi_render_points_moments_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                                     const float* d_points, const float* d_normals, uint32_t rows_per_pixel,
                                     uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4, void* d_compact_m2,
                                     void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);
int  mi_bake_lightmap_moments(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                              float offset, float* out_m2, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig,
                              int32_t* out_triangle, mi_stats* stats);

/* ---- lightmap variance: variance-guided finishing (added within ABI version 5: detect by symbol lookup) ----
 * mi_lightmap_finish with a colour weight that follows each texel's own noise instead of one sigma_color for the whole atlas: a 16-sample
 *   bake has texels in direct light that are nearly converged beside texels in deep indirect light whose standard error is tens of times
 *   larger, and one sigma either leaves the second kind noisy or blurs real detail in the first.  Here the weight's width is sigma_color
 *   standard errors of the texel itself, the variance filtered along with the image (as SVGF does).
 *   These are the semantics of lightmap_finish_var (Python), which is the definition; the result equals the helper's BIT FOR BIT: pure
 *   f32, every operation one of + - * /, sqrtf, fabsf, fmaxf, comparisons and exact int-to-float conversions, in the order written here,
 *   no fused multiply-add, IEEE division and square root.  No scene is needed.
 * Layout: mi_lightmap_finish's, and `m2` [H][W][3] f32 is the bake's out_m2, `samples` its aa_sample_count S (2 .. 65535), out_var
 *   [H][W] f32 (may be NULL).  The coverage rule, the tap order, h, wn, wp, the reach test, the centre tap's exemption and the dilation
 *   are mi_lightmap_finish's, letter for letter.  New:
 * Initial variance of the mean, covered texels: v_c = fmaxf(0, m2_c - mean_c * mean_c) / (float)(S - 1), V = (v_r + v_g) + v_b; empty
 *   texels V = +0.0.  The difference cancels in f32: V is meaningless where the true noise is below about 1e-3 of the mean (it may come
 *   out as 0 or as rounding noise of the order mean^2 * 6e-8 / S); color_floor exists for that case.
 * Per level (s = 2^i, ping-pong, never in place), for a covered texel p:
 *   blur: bs = sum g V_q, bw = sum g over the nine neighbours q = p + (dx, dy) at step 1 WHATEVER s is, dy outer -1 .. 1, dx inner
 *     -1 .. 1, both sums from +0.0; a neighbour counts when it lies in the image and is covered; g = G3[dy+1] * G3[dx+1],
 *     G3 = { 1/4, 1/2, 1/4 }.  sd = sqrtf(bs / bw), den = sigma_color * sd + color_floor.
 *   a-trous: wc = fmaxf(0, 1 - dc / den), dc as mi_lightmap_finish's from the current level's colours, den taken at p only and NOT
 *     divided by s; w = ((h wn) wp) wc; sw = sw + w; sc[k] = sc[k] + w c_q[k]; sv = sv + (w * w) * V_q.  The texel becomes sc / sw and
 *     its variance sv / (sw * sw).
 *   color_floor = +inf turns the colour weight off (1 - dc / inf == 1): the image is then mi_lightmap_finish's with sigma_color = +inf,
 *   bit for bit.
 * out_var: the final V for covered texels, +0.0 elsewhere, texels filled by the dilation included.  levels == 0 gives the masked copy
 *   and the initial V.
 * Non-finite values never fault; they give unspecified values only for texels within Chebyshev radius 2 (2^levels - 1) + levels + dilate
 *   (the blur widens each level's reach by one); every other texel keeps the bits of the clean run.  No address depends on a table value.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): NULL image, m2, points, normals or out_image;
 *   width or height of 0 or above 32768; levels > 8, normal_power_log2 > 7, dilate > 256; samples < 2 or > 65535; a sigma_plane or reach
 *   that is NaN or <= 0; a sigma_color that is NaN, infinite or < 0; a color_floor that is NaN or <= 0 (+inf is legal).
 * Scratch: mi_lightmap_finish's, and three [H][W] f32 planes (two variances, the denominators) in a buffer the context owns (grown on
 *   demand, freed with the context, never the buffers mi_reserve sized; MI_ERR_OOM).  lmv_init once, lmv_blur and lmv_atrous per level
 *   (one 32 x 32 tile per block, the taps straight from HBM / L2), lmf_dilate per pass; mi_last_kernel_ms reports their sum.
 * mi_lightmap_finish_var: HOST pointers, blocking; the tables pass through a buffer the context owns; out_image may alias image.
 * mi_lightmap_finish_var_device: DEVICE pointers on ctx's device.  Queues on `stream` and does not synchronise, except when it has to
 *   grow its scratch.  An out_image or out_var that overlaps image, m2, points or normals is MI_ERR_INVALID. */
int  mi_lightmap_finish_var(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2, uint32_t samples,
                            const float* points, const float* normals, uint32_t levels, uint32_t normal_power_log2, float sigma_plane,
                            float reach, float sigma_color, float color_floor, uint32_t dilate, float* out_image, float* out_var,
                            uint8_t* out_valid);
int  mi_lightmap_finish_var_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2, uint32_t samples,
                                   const float* points, const float* normals, uint32_t levels, uint32_t normal_power_log2,
                                   float sigma_plane, float reach, float sigma_color, float color_floor, uint32_t dilate, float* out_image,
                                   float* out_var, uint8_t* out_valid, void* stream);

/* ---- adaptive lightmap bake: further samples where the variance asks (added within ABI version 5: detect by symbol lookup) ----
 * A bake spends the same aa_sample_count on a texel in direct light, converged after 16 samples, as on one lit only through two bounces.
 *   The second moments say which texels are which; these calls act on it without touching the wavefront pipeline: a refinement round is
 *   an ordinary mi_render_points_moments render of a COMPACT point table that holds the selected texels only.  New are the selection, the
 *   compaction, the merge, and a finish that takes per-texel counts.  The numpy helpers lightmap_select, lightmap_gather and lightmap_merge
 *   (Python) are the definitions; the results equal them BIT FOR BIT: pure f32, every operation one of + - * /, sqrtf, fabsf, fmaxf,
 *   comparisons and exact int-to-float conversions, in the order written here, no fused multiply-add, IEEE division and square root, no
 *   float atomics, nothing summed across threads but integer counts: no result depends on scheduling.  No scene is needed.  No address
 *   depends on a table value except through the index list, whose entries are tested against W * H before use.
 * mi_lightmap_select: `image` and `m2` [H][W][3] f32 are a bake's mean and mean of squares, `counts` [H][W] u32 the samples behind each
 *   texel, `normals` [H][W][3] the centre table (mi_lightmap_finish's coverage rule: an all-zero normal is an empty texel, never
 *   selected); target_rel and target_abs are >= 0 (+inf is legal).
 *   Per covered texel with n = counts: n >= 2 gives v_c = fmaxf(0, m2_c - mean_c * mean_c) / (float)(n - 1), V = (v_r + v_g) + v_b
 *   (mi_lightmap_finish_var's initial variance with the texel's own n); n < 2 gives V = +inf: the texel has no information and is always
 *   selected.  Empty texels V = +0.0.  Then sd = sqrtf(bs / bw) with mi_lightmap_finish_var's blur, sums and order (the nine step-1
 *   neighbours that lie in the image and are covered): a dark texel whose few samples all missed the light is not judged converged
 *   beside bright neighbours.  With lum = (fabsf(mean_r) + fabsf(mean_g)) + fabsf(mean_b) the texel is selected when
 *   sd > target_rel * lum + target_abs (one multiply, one add).
 *   out_index [capacity] u32: the selected texel numbers y * W + x, ascending; out_count [1] u32: the number of selected texels, which
 *   may exceed capacity: the list then holds the lowest `capacity` of them.  Entries at and behind min(out_count, capacity) are not
 *   written.  out_index may be NULL when capacity is 0.  out_error [H][W] f32 (may be NULL): sd, +0.0 on empty texels.
 *   A NaN or infinite texel of image or m2 changes the selection within Chebyshev distance 1 only.  Kernels: lmv_init_counts, lma_mark
 *   (blur, threshold and the count of every block of 1024 consecutive texels, by wave ballot), lma_scan (the prefix of the block counts),
 *   lma_fill (every block writes its texels at its offset).
 * mi_lightmap_gather: `index` [n] lists texels; `points` and `normals` are [rows][H][W][3] f32 (rows in 1 .. 65535); the outputs are the
 *   compact tables [rows][ch][cw][3], ch = ceil(n / cw), cw in 1 .. 32768, ch in 1 .. 32768 (so n >= 1).  Entry i goes to slot
 *   (i / cw, i % cw) of every row; the slots at or behind n are all zero, the empty-texel mark: mi_render_points traces nothing for them.
 *   An index >= W * H gives an empty slot; the table is not read through it.
 * mi_lightmap_merge: `mean` and `m2_round` [ch][cw][3] f32 (their first n slots are read) are the mean and mean of squares of a round
 *   of round_samples = S' (1 .. 65535) samples of the n listed texels; `image`, `m2` [H][W][3] f32 and `counts` [H][W] u32 are read AND
 *   written.  For each listed texel with count n0, per channel: image = ((float)n0 * image + (float)S' * mean') / (float)(n0 + S'), m2
 *   likewise, counts = n0 + S'.  Every other texel keeps its bits; an index >= W * H is skipped; n == 0 does nothing.  One lane per
 *   entry: a list with a texel twice gives unspecified values for that texel only (the device form) and is MI_ERR_INVALID in the host
 *   form, which can check.  Counts above 2^24 give unspecified values for that texel.
 * mi_lightmap_finish_var_counts: mi_lightmap_finish_var letter for letter with `counts` [H][W] u32 in place of `samples`: the initial
 *   variance divides by (float)(n - 1) with the texel's own n, and n < 2 gives V = +0.0 there.  A plane that holds one value S
 *   everywhere gives mi_lightmap_finish_var's result for samples = S, bit for bit.  The device form refuses outputs that overlap counts
 *   as well.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): a NULL pointer other than out_error, out_var,
 *   out_valid (and out_index at capacity 0); width or height of 0 or above 32768; a target that is NaN or negative; rows, cw, ch or
 *   round_samples outside their ranges; mi_lightmap_finish_var's for the finish.
 * Scratch: one f32 plane, one u8 plane and two words per 1024 texels for select, in a buffer the context owns (grown on demand, freed
 *   with the context, never the buffers mi_reserve sized; MI_ERR_OOM); mi_last_kernel_ms reports the sum of the call's kernels.
 * The forms without _device take HOST pointers, block, and pass their tables through a buffer the context owns; the _device forms take
 *   DEVICE pointers on ctx's device, queue on `stream` and do not synchronise, except when they have to grow their scratch. */
int  mi_lightmap_select(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2, const uint32_t* counts,
                        const float* normals, float target_rel, float target_abs, uint32_t capacity, uint32_t* out_index,
                        uint32_t* out_count, float* out_error);
int  mi_lightmap_select_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2, const uint32_t* counts,
                               const float* normals, float target_rel, float target_abs, uint32_t capacity, uint32_t* out_index,
                               uint32_t* out_count, float* out_error, void* stream);
int  mi_lightmap_gather(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* index,
                        const float* points, const float* normals, uint32_t cw, float* out_points, float* out_normals);
int  mi_lightmap_gather_device(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t rows, uint32_t n, const uint32_t* index,
                               const float* points, const float* normals, uint32_t cw, float* out_points, float* out_normals,
                               void* stream);
int  mi_lightmap_merge(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t n, const uint32_t* index, const float* mean,
                       const float* m2_round, uint32_t round_samples, float* image, float* m2, uint32_t* counts);
int  mi_lightmap_merge_device(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t n, const uint32_t* index, const float* mean,
                              const float* m2_round, uint32_t round_samples, float* image, float* m2, uint32_t* counts, void* stream);
int  mi_lightmap_finish_var_counts(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2,
                                   const uint32_t* counts, const float* points, const float* normals, uint32_t levels,
                                   uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color, float color_floor,
                                   uint32_t dilate, float* out_image, float* out_var, uint8_t* out_valid);
int  mi_lightmap_finish_var_counts_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const float* m2,
                                          const uint32_t* counts, const float* points, const float* normals, uint32_t levels,
                                          uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color, float color_floor,
                                          uint32_t dilate, float* out_image, float* out_var, uint8_t* out_valid, void* stream);

/* mi_bake_lightmap_adaptive: mi_bake_lightmap_moments with refinement rounds.  HOST pointers, blocking.  out_counts [H][W] u32 and out_m2
 *   are required; cam->aa_sample_count is ignored.
 * Round 0 is mi_bake_lightmap_moments with aa_sample_count = first_samples and seed opts->seed; every texel's count is first_samples.
 * Round r = 1 .. max_rounds: mi_lightmap_select on the device with capacity 2^25; the one count is read back, and 0 ends the bake;
 *   mi_lightmap_gather with cw = 1024, without MI_LM_JITTER from the centre table (mi_lightmap_texels with rows = 1), with MI_LM_JITTER
 *   from a fresh mi_lightmap_texels table of round_samples rows made with seed opts->seed + r; the compact table is rendered exactly as
 *   mi_render_points_moments does for a camera of 1024 x ch with aa_sample_count = round_samples and seed opts->seed + r (u32 wrap: a
 *   different seed per round keeps each round's samples independent of all earlier ones under the existing stream keys); mi_lightmap_merge.
 * Outputs: the merged mean (out_rgb_f32), the merged out_m2 and out_counts; out_rgb_u8 is mi_tonemap_device of the merged mean; out_sig
 *   and out_triangle are round 0's; stats->samples counts the slots of all rounds (W * H * first_samples + 1024 * ch * round_samples
 *   per round), kernel_ms and total_ms are sums.  The result is BIT FOR BIT what the public calls above and mi_render_points_moments
 *   give when composed in that order: nothing is hidden in this call.
 * Selection looks at the running estimate, so the merged mean is consistent, not strictly unbiased: a texel whose first samples
 *   happen to agree stops early with whatever they agree on.  This is a documented property, not a defect; the blur of the variance and
 *   the n < 2 rule bound it.
 * MI_ERR_INVALID: every refusal of mi_bake_lightmap_moments, and first_samples < 2, round_samples == 0, either above 65535,
 *   first_samples + max_rounds * round_samples > 2^24 (a count stays exact in f32), a NaN or negative target, a NULL adaptive, out_m2
 *   or out_counts.  Nothing is launched.  The planes, the list and the compact tables live in buffers the context owns. */
typedef struct mi_lightmap_adaptive {
    uint32_t first_samples;     /* round 0: samples of every texel (2 .. 65535)           */
    uint32_t round_samples;     /* samples a selected texel gets per round (1 .. 65535)   */
    uint32_t max_rounds;        /* refinement rounds at most (0: mi_bake_lightmap_moments) */
    float    target_rel;        /* a texel is done when sd <= target_rel * lum + target_abs */
    float    target_abs;
} mi_lightmap_adaptive;         /* 20 bytes */
int  mi_bake_lightmap_adaptive(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                               float offset, const mi_lightmap_adaptive* adaptive, uint32_t* out_counts, float* out_m2,
                               float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, int32_t* out_triangle, mi_stats* stats);

/* ---- light probes: SH L2 radiance probes with the directions drawn on the GPU (added within ABI version 5: detect by symbol lookup) ----
 * mi_render_points without normals and with a second output.  One "pixel" is one probe, a point in free space; its samples leave it in
 *   directions uniform over the whole sphere, and beside their mean the call returns the radiance field's projection onto the nine real
 *   spherical harmonics of order <= 2 per colour channel, from which the irradiance for any normal is a dot product (sh9_irradiance in
 *   Python).  A caller with n probes uses W = n, H = 1, or any grid that holds them.
 * Layout: `points` is [rows_per_pixel][H][W][3] f32, W x H = cam->screen_width x screen_height, probe (row, y, x) at ((row*H + y)*W + x)*3
 *   (indexed in 64 bits); rows_per_pixel is 1 or aa_sample_count, as for the point table.
 * Two streams per sample s of probe (x, y), the point table's keys:
 *   direction: (seed, W*H + y*W + x, s), fresh: d = rand_sphere_vec(), what Isotropic::scatter (materials.rs:158-166) returns on that
 *     stream.  d is NOT normalised (|d| <= 1); rejection from the cube makes its direction uniform on the sphere, pdf 1 / (4 pi).
 *   path: (seed, y*W + x, s), fresh: L_s = Scene::shade_ray(Ray(p, d), 0), t_min = 0.001 and t_max = cam->max_trace_dist in units of |d|.
 *   Hence mi_render_probes(points) has the mean image of mi_render_rays(points, d) for the table d of those directions, bit for bit.
 * Plain outputs: the mean (f32), u8 and signature outputs of mi_render_points, made by the same reduction.
 * SH output: out_sh is [H][W][9][3] f32, c_k = (4 pi / S) * sum_s L_s * Y_k(u_s), u_s = d_s / |d_s|, S = aa_sample_count, with the real
 *   basis in this order (constants rounded to f32):
 *     Y_0 = 0.28209479177387814          Y_1 = 0.4886025119029199 y       Y_2 = 0.4886025119029199 z      Y_3 = 0.4886025119029199 x
 *     Y_4 = 1.0925484305920792 x y       Y_5 = 1.0925484305920792 y z     Y_6 = 0.31539156525252005 (3 z^2 - 1)
 *     Y_7 = 1.0925484305920792 x z       Y_8 = 0.5462742152960396 (x^2 - y^2)
 *   Each of the 27 sums is accumulated in f32 in sample order from +0.0 (one multiply and one add per sample, not fused), and scaled
 *   once at the end by 12.566370614359172f / (float)S: out_sh is bit-identical across max_state_bytes, ranks, MI_OPT_* flags and
 *   progressive splits.
 * No empty-probe marker: a probe has no normal, and (0, 0, 0) is a legitimate position.  A non-finite point gives unspecified values
 *   for that probe only; it never faults and changes no other probe's bits (no address depends on a table value).  A d with
 *   dot(d, d) == 0 (all three draws exactly 0) has no direction: that sample's contribution to the 27 sums is unspecified (NaN).
 * Everything else is mi_render_points', word for word: the camera fields read and ignored, the refusals (NULL table, rows_per_pixel,
 *   path_samples != 1, MI_SHADE_PHONG, a variant other than DEFAULT / WAVEFRONT, no scene, rank / world), masks OFF (entry 7 of
 *   mi_last_pipeline_counts is 0), mi_reserve, max_state_bytes, stats->samples = W*H*aa_sample_count.  Entry 7 of mi_last_pipeline_ms
 *   is the time of the SH reduction (wf_reduce_sh), which runs behind wf_reduce in every batch.
 * mi_render_probes: HOST pointers, blocking, rank / world 0 / 1; out_sh is required (MI_ERR_INVALID if NULL), the other outputs may be NULL.
 * mi_render_probes_device: DEVICE pointers; the sample range, the accumulator and the rank / world rules are mi_render_rays_device's.
 *   d_compact_sh is [tiles_padded][1024][27] f32 in the compact tile-major layout ([9][3] per slot), output AND running accumulator: the
 *   call with sample_begin == 0 starts the sums from zero (the buffer need not be cleared), later calls add to it, the call that ends at
 *   aa_sample_count applies the scale; it may be copied out and back between calls.  Slots outside the image and padding slots are
 *   written as zeros.  d_compact_sh == NULL is legal and gives the plain outputs only.  mi_multi_* takes no table. */
int  mi_render_probes(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                      const float* points, uint32_t rows_per_pixel, float* out_sh,
                      float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);
int  mi_render_probes_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                             const float* d_points, uint32_t rows_per_pixel,
                             uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4, void* d_compact_sh,
                             void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);

/* ---- irradiance volumes: SH L2 probe grids sampled at surface points (added within ABI version 5: detect by symbol lookup) ----
 * What uses mi_render_probes' result: the grid of radiance probes that probe_grid (Python) places in a box is interpolated at arbitrary
 *   surface points and convolved with the clamped cosine lobe about each point's normal, giving the irradiance E(n) there (constant
 *   radiance L gives pi L; divide by pi and multiply by the albedo for a Lambertian surface).  Millions of points per call: the vertices of
 *   moving meshes, or the texels of an atlas table (mi_lightmap_texels) for a preview lightmap in milliseconds.  No scene is needed.
 * These are the semantics of probe_volume_sample (Python), which is the definition; the result equals the helper's BIT FOR BIT: pure
 *   f32, every operation one of + - * /, sqrtf, floorf, fminf, fmaxf, comparisons and exact int-to-float conversions, in the order
 *   written here, no fused multiply-add, IEEE division and square root.
 * Volume: `sh` is exactly the first n_probes = nx ny nz records of mi_render_probes' out_sh for a probe_grid table (the flat prefix of
 *   [H][W][9][3] is [n_probes][9][3]: pass that buffer as it is).  `valid` marks probes that take no part (inside geometry, say); the
 *   caller computes it.  Grid constants per axis a, in f32: cell_a = (hi_a - lo_a) / (float)n_a, inv_a = (float)n_a / (hi_a - lo_a).
 * Prepared record of probe q: r[k][c] = sh[q][k][c] * K_k, rounded once; K_k is the cosine-lobe factor times the basis constant, rounded
 *   from f64 to f32: K_0 = 0.886226925452758, K_1..3 = 1.0233267079464885, K_4 = K_5 = K_7 = 0.8580855308097834,
 *   K_6 = 0.24770795610037571, K_8 = 0.4290427654048917.
 * Normal (nx, ny, nz): all-zero (either sign of zero) is the empty-texel mark of mi_render_points: the output is +0.0 and the weight 0, so
 *   an atlas table is a legal input as it stands.  Otherwise l = sqrtf((nx nx + ny ny) + nz nz), x = nx / l, y = ny / l, z = nz / l and
 *   b = { 1, y, z, x, x*y, y*z, 3*(z*z) - 1, x*z, x*x - y*y }.
 * Cell, per axis: g = (p_a - lo_a) * inv_a - 0.5f; g = fminf(fmaxf(g, 0), (float)(n_a - 1)) (which also keeps every index in range for
 *   NaN and infinite points); i0 = min((int)floorf(g), max(n_a - 2, 0)); f = g - (float)i0.  Outside the box the edge cells extend.
 * Eight corners, dz outer, dy, dx inner: index i_a = min(i0_a + d_a, n_a - 1); w_a = d_a ? f_a : 1 - f_a; w = (w_x * w_y) * w_z;
 *   w = 0 when valid[q] == 0.  With MI_PV_NORMAL_WEIGHT: D_a = (lo_a + ((float)i_a + 0.5f) * cell_a) - p_a,
 *   dd = (Dx Dx + Dy Dy) + Dz Dz, and when dd > 0: t = ((Dx x + Dy y) + Dz z) / sqrtf(dd), h = (t + 1) * 0.5f, w = w * (h*h + 0.2f)
 *   (a probe behind the surface counts less, never nothing; w is unchanged when dd == 0).  Then, summed left to right,
 *   e[c] = b0*r[0][c] + b1*r[1][c] + ... + b8*r[8][c];  acc[c] = acc[c] + w * e[c];  sw = sw + w.
 * Result: out_irradiance[c] = acc[c] / sw when sw > 0, else +0.0; out_weight = sw (0: every corner was invalid).
 * A non-finite point or normal gives an unspecified value for that point only; it never faults and changes no other point's bits.  The
 *   result does not depend on scheduling: no atomics, nothing is summed across threads.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): a NULL volume, sh, points, normals or
 *   out_irradiance; a count of 0 or above 1024; more than 2^22 probes; an unknown flag; a lo or hi that is not finite, or hi[a] <= lo[a].
 *   n_points == 0 is MI_OK and launches nothing.
 * Scratch: one 112-byte record per probe (28 floats: the 27 products and the validity as 0.0 / 1.0) in a buffer the context owns (grown on
 *   demand, freed with the context, never the buffers mi_reserve sized; MI_ERR_OOM if it cannot be allocated); the host form keeps the
 *   uploaded sh and valid behind it.  Two kernels per call (the records, then one lane per point); mi_last_kernel_ms reports their sum.
 * mi_probe_volume_sample: HOST pointers (sh and valid included), blocking; the points go through the ray queries' chunk buffer.
 * mi_probe_volume_sample_device: sh, valid, points, normals and the outputs are DEVICE pointers on ctx's device (the struct itself is
 *   host memory).  Queues on `stream` and does not synchronise, except when it has to grow its scratch.  The records belong to the
 *   context: calls on different streams of one context must not overlap. */
typedef struct mi_probe_volume {
    float          lo[3];           /* the box probe_grid was given                                  */
    float          hi[3];
    uint32_t       counts[3];       /* nx, ny, nz: probe (i,j,k) has number (k*ny + j)*nx + i        */
    uint32_t       flags;           /* MI_PV_* bits                                                  */
    const float*   sh;              /* [n_probes][9][3] f32, mi_render_probes' out_sh order          */
    const uint8_t* valid;           /* [n_probes] bytes, 0 = probe takes no part; NULL = all valid   */
} mi_probe_volume;              /* 56 bytes */
int  mi_probe_volume_sample(mi_ctx* ctx, const mi_probe_volume* volume, uint32_t n_points, const float* points, const float* normals,
                            float* out_irradiance, float* out_weight);
int  mi_probe_volume_sample_device(mi_ctx* ctx, const mi_probe_volume* volume, uint32_t n_points, const float* points, const float* normals,
                                   float* out_irradiance, float* out_weight, void* stream);

/* ---- directional lightmaps: per-texel SH L2 bake, finish and evaluation (added within ABI version 5: detect by symbol lookup) ----
 * What mi_render_points stores per texel is the plain mean of its samples over directions UNIFORM on the hemisphere (sample_hemisphere's
 *   pdf is 1 / (2 pi)): the mean incoming radiance, not the irradiance, and fixed to the table's normal.  These calls store the radiance
 *   field's projection onto the nine real SH of order <= 2 per texel instead, from which mi_lightmap_sh_eval gives the cosine-weighted
 *   irradiance E(n') for whatever normal n' the caller passes: the table's own normal for a plain irradiance map, a normal-mapped one
 *   for the detail a lightmap is too coarse to hold.
 * mi_render_points_sh / mi_render_points_sh_device / mi_bake_lightmap_sh: mi_render_points / _device / mi_bake_lightmap with one more
 *   output, out_sh [H][W][9][3] f32: c_k = (2 pi / S) * sum_s L_s * Y_k(u_s), u_s = d_s / |d_s|, d_s the direction the point table's
 *   direction stream (seed, W*H + y*W + x, s) gives sample s, L_s the sample the mean is made of, S = aa_sample_count; basis, order and
 *   constants are mi_render_probes'.  Each of the 27 sums is accumulated in f32 in sample order from +0.0 (one multiply and one add per
 *   sample, not fused) and scaled once at the end by 6.283185307179586f / (float)S: out_sh is bit-identical across max_state_bytes,
 *   ranks, MI_OPT_* flags and progressive splits.  The directions cover the hemisphere about the table's normal only:
 *   radiance from below that horizon is not sampled and counts as zero (constant radiance L gives E(n) = pi L at the table's normal).
 *   Empty texels: a sample whose row's normal is all-zero (either sign of zero) adds nothing and draws nothing; a texel whose rows are
 *   all empty is 27 x +0.0; with a jittered table (rows == S) a texel may have some empty rows, and the scale stays 2 pi / S, as the
 *   mean's divisor stays S.  A non-finite point or normal gives unspecified values for that texel's 27 floats only.
 *   Plain outputs: the mean (f32), u8 and signature outputs are mi_render_points' / mi_bake_lightmap's BIT FOR BIT: the SH sums are a
 *   further reduction (wf_reduce_psh) of the same sample slots behind wf_reduce in every batch, which reads the normal table again; no
 *   other kernel runs differently, and it never runs in one render with wf_reduce_m2.  Entry 7 of mi_last_pipeline_ms is its time after
 *   these calls.  Everything else is mi_render_points' / mi_bake_lightmap's, word for word: the tables, the two streams, the camera
 *   fields, the refusals, masks OFF, mi_reserve, max_state_bytes, stats.
 *   Host forms: out_sh is required (MI_ERR_INVALID if NULL, checked first), the other outputs may be NULL; the records live in the buffer
 *   mi_render_probes' do.  Device form: d_compact_sh is [tiles_padded][1024][27] f32, output AND running accumulator with
 *   mi_render_probes_device's rules: the call with sample_begin == 0 starts the sums from zero (the buffer need not be cleared), later
 *   calls add to it, the call that ends at aa_sample_count applies the scale; it may be copied out and back between calls; slots outside
 *   the image and padding slots are written as zeros.  d_compact_sh == NULL is exactly mi_render_points_device.
 * mi_lightmap_finish_sh / _device: mi_lightmap_finish for images of [H][W][9][3] records (`sh`, `out_sh`): the same guides (centre
 *   table), levels, taps and tap order, h, wn, wp, reach test and centre-tap exemption, dilation, parameter ranges and refusals.  The
 *   colour distance dc is taken from the three k = 0 coefficients of the current level; one weight w = ((h wn) wp) wc per tap serves
 *   all 27 channels, sc[j] = sc[j] + w c_q[j], and the record becomes sc[j] / sw.  The dilation sums all 27 channels over the same
 *   neighbours in the same order with one count.  Empty texels are 27 x +0.0 at every level; out_valid is mi_lightmap_finish's.
 *   lightmap_finish_sh (Python) is the definition; the result equals it BIT FOR BIT.  Hence the k = 0 plane of the result is
 *   mi_lightmap_finish of the k = 0 plane alone, and with sigma_color = +inf every plane k is mi_lightmap_finish of that plane.
 *   Scratch: two [H][W][27] f32 images and two byte masks in a buffer the context owns (grown on demand, freed with the context, never
 *   the buffers mi_reserve sized; MI_ERR_OOM); one kernel per level and per pass (lsh_atrous: one 32 x 32 tile per block, the taps
 *   straight from HBM / L2), mi_last_kernel_ms reports their sum.  The host form blocks and out_sh may alias sh; the device form queues
 *   on `stream`, does not synchronise except to grow its scratch, and refuses an out_sh that overlaps sh, points or normals.
 * mi_lightmap_sh_eval / _device: `sh` [n][9][3], `normals` [n][3], out_irradiance [n][3]; an atlas is n = W*H with the flat buffers as
 *   they stand.  An all-zero normal gives +0.0 (an atlas's normal table is a legal input).  Otherwise l, x, y, z and b[9] are
 *   mi_probe_volume_sample's, r_k = sh_k * K_k rounded once (its K_k), e[c] = b0*r[0][c] + ... + b8*r[8][c] summed left to right: the
 *   value mi_probe_volume_sample gives for a 1 x 1 x 1 volume holding that record, bit for bit.  lightmap_sh_eval (Python) is the
 *   definition.  The result is NOT clamped: SH ringing can take it slightly below zero beside strong directional light.  One lane per
 *   point; mi_last_kernel_ms reports the kernel.  NULL sh, normals or out_irradiance are MI_ERR_INVALID (checked before the context);
 *   n == 0 is MI_OK and launches nothing.  The host form passes its arrays through a buffer the context owns. */
int  mi_render_points_sh(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                         const float* points, const float* normals, uint32_t rows_per_pixel, float* out_sh,
                         float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);
int  mi_render_points_sh_device(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts,
                                const float* d_points, const float* d_normals, uint32_t rows_per_pixel,
                                uint32_t sample_begin, uint32_t sample_end, void* d_accum_f32x4, void* d_compact_sh,
                                void* d_compact_f32, void* d_sig_u32, void* stream, mi_stats* stats);
int  mi_bake_lightmap_sh(mi_ctx* ctx, const mi_camera_desc* cam, const mi_render_opts* opts, const mi_mesh* mesh, uint32_t flags,
                         float offset, float* out_sh, float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig,
                         int32_t* out_triangle, mi_stats* stats);
int  mi_lightmap_finish_sh(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const float* points, const float* normals,
                           uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                           uint32_t dilate, float* out_sh, uint8_t* out_valid);
int  mi_lightmap_finish_sh_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const float* points, const float* normals,
                                  uint32_t levels, uint32_t normal_power_log2, float sigma_plane, float reach, float sigma_color,
                                  uint32_t dilate, float* out_sh, uint8_t* out_valid, void* stream);
int  mi_lightmap_sh_eval(mi_ctx* ctx, uint32_t n, const float* sh, const float* normals, float* out_irradiance);
int  mi_lightmap_sh_eval_device(mi_ctx* ctx, uint32_t n, const float* sh, const float* normals, float* out_irradiance, void* stream);

/* ---- lightmap lookup: a finished lightmap read at uv points (added within ABI version 5: detect by symbol lookup) ----
 * The last step of the lightmap pipeline: mi_intersect_rays gives, per ray, out_uv (RayHit.tex_coords) and the shading normal; these calls
 *   give the lightmap there.  mi_lightmap_sample interpolates an [H][W][channels] f32 image, channels 3 (mi_lightmap_finish's) or 27
 *   (mi_lightmap_finish_sh's records, flat); mi_lightmap_sh_sample reads [H][W][9][3] records and gives the irradiance at each point's own
 *   normal in one pass.  `valid` is the finish calls' out_valid as it stands ([H][W] bytes, 0 = the texel takes no part; NULL = all
 *   valid).  lightmap_sample and lightmap_sh_sample (Python) are the definitions; the results equal them BIT FOR BIT: pure f32, every
 *   operation one of + - * /, sqrtf, floorf, fminf, fmaxf, comparisons and exact int-to-float conversions, in the order written here, no
 *   fused multiply-add.  No scene is needed; nothing depends on scheduling (no atomics, nothing summed across threads).
 * Bilinear (flags == 0), per point (u, v): gx = u * (float)W - 0.5f, gy = (1 - v) * (float)H - 0.5f (row 0 is v = 1: Texture::sample's
 *   flip, texture.rs:29).  Per axis g = fminf(fmaxf(g, 0), (float)(n - 1)) — fmaxf sends a NaN to 0, so every index stays in range for NaN
 *   and infinite coordinates — i0 = min((int)floorf(g), max(n - 2, 0)), f = g - (float)i0, i1 = min(i0 + 1, n - 1): the clamp wrap mode,
 *   the only one.  Four taps, dy outer, dx inner: w = wx[dx] * wy[dy] with w_a = { 1 - f, f }.  A tap takes part when w > 0 and its texel
 *   is valid; a tap that takes no part is not read.  acc[c] = acc[c] + w * t[c] and sw = sw + w from +0.0; out[c] = acc[c] / sw when
 *   sw > 0, else +0.0; out_weight = sw (1 within rounding inside a chart, smaller where invalid texels were left out, 0: nothing to read).
 * MI_LS_NEAREST, the reference's own addressing (texture.rs:28-29) in f32: x = 0 when u is a NaN (Rust's saturating cast), else
 *   x = min((int)(fminf(fmaxf(u, 0), 0.999f) * (float)W), W - 1); y = 0 when v is a NaN, else
 *   y = min((int)((1 - fminf(fmaxf(v, 0), 0.999f)) * (float)H), H - 1).  The output is that texel's values as they stand with weight 1,
 *   or +0.0 with weight 0 when the texel is invalid.  No NaN reaches a float-to-int conversion.
 * mi_lightmap_sh_sample: an all-zero normal (either sign of zero) gives +0.0 and weight 0.  Otherwise x, y, z, b[9] and K_k are
 *   mi_lightmap_sh_eval's; per tap that takes part e[c] = b0*(sh[0][c]*K_0) + ... + b8*(sh[8][c]*K_8) summed left to right, then
 *   acc[c] = acc[c] + w * e[c], sw = sw + w, out_irradiance[c] = acc[c] / sw: mi_probe_volume_sample's order, three accumulators and
 *   never an interpolated record.  With MI_LS_NEAREST out_irradiance is e of the one texel: mi_lightmap_sh_eval of that record, bit for
 *   bit.  NOT bit-equal to mi_lightmap_sample at 27 channels followed by mi_lightmap_sh_eval, which rounds in another order.
 * Non-finite input: non-finite uv, normals or texel values never fault; they spoil only the points whose taking-part taps touch them (a
 *   non-finite uv behaves as the clamped coordinate it becomes; a non-finite normal spoils its own point).  No address depends on anything
 *   but the clamped indices.  Texels behind valid == 0 may hold anything: they are never read.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): a NULL image / sh, uv, normals or out /
 *   out_irradiance (valid and out_weight may be NULL); width or height 0 or above 32768; channels other than 3 or 27; unknown flag bits;
 *   in the _device forms an output that overlaps an input.  n == 0 is MI_OK and launches nothing.
 * Host forms: HOST pointers, blocking; the arrays pass through a buffer the context owns.  _device forms: DEVICE pointers on ctx's device;
 *   they queue one kernel on `stream`, do not synchronise and need no scratch, so calls on different streams may overlap;
 *   mi_last_kernel_ms reports the kernel.  Indices are 64-bit: a 32768 x 32768 table of records is legal. */
int  mi_lightmap_sample(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                        uint32_t n, const float* uv, uint32_t flags, float* out, float* out_weight);
int  mi_lightmap_sample_device(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                               uint32_t n, const float* uv, uint32_t flags, float* out, float* out_weight, void* stream);
int  mi_lightmap_sh_sample(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t n,
                           const float* uv, const float* normals, uint32_t flags, float* out_irradiance, float* out_weight);
int  mi_lightmap_sh_sample_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t n,
                                  const float* uv, const float* normals, uint32_t flags, float* out_irradiance, float* out_weight,
                                  void* stream);

/* ---- lightmap mips: the coverage-aware pyramid of a finished lightmap and the trilinear lookup that reads it (added within ABI
 *   version 5: detect by symbol lookup) ----
 * A lookup whose footprint spans many texels (distant surfaces, grazing angles) aliases at level 0.  mi_lightmap_mips makes the levels
 *   above it; a plain 2 x 2 box would pull in the texels no pass filled, so every level carries the fraction of its footprint that is
 *   valid and averages over exactly those texels.  lightmap_mips, lightmap_sample_lod and lightmap_sh_sample_lod (Python) are the
 *   definitions; the results equal them BIT FOR BIT under the contract of the lookup section above: pure f32, one rounding per operation,
 *   in the order written here, no fused multiply-add, nothing summed across threads.
 * The layout, one rule: `levels` counts level 0.  Level l is W_l x H_l with W_l = (W + 2^l - 1) >> l and H_l likewise (ceil halving):
 *   texel (x, y) of level l covers exactly the level-0 texels [x 2^l, (x+1) 2^l) x [y 2^l, (y+1) 2^l) that lie inside the image, for
 *   any size.  The full chain has 1 + ceil(log2(max(W, H))) levels (16 at 32768) and ends at 1 x 1.  levels == 0 means the full chain;
 *   levels above the full chain is refused.  Levels 1 .. L-1 are stored tightly, one after the other, level 1 first:
 *   mips [sum W_l H_l][channels] f32, mip_valid [sum W_l H_l] u8, mip_coverage [sum W_l H_l] f32.  Level 0 is not copied.
 * mi_lightmap_mips: cov_0 = 1.0 where valid (valid == NULL: everywhere), else 0.0.  For l >= 1 texel (x, y) has the children
 *   (2y + dy, 2x + dx) of level l-1, dy outer, dx inner.  A child takes part when it lies inside level l-1 and its c = cov_(l-1) > 0; a
 *   child that takes no part is not read.  acc[k] = acc[k] + c * t[k] and sc = sc + c from +0.0; out[k] = acc[k] / sc when sc > 0, else
 *   +0.0; cov_l = sc * 0.25f; valid_l = cov_l > 0.  So cov_l is the fraction of the texel's level-0 footprint that is valid and out
 *   the mean over exactly those texels.  cov_l is exact while 4^l <= 2^24, that is l <= 12; beyond that it is rounded as written, and
 *   the helper remains the definition.  Texels behind valid == 0 may hold anything; a non-finite valid texel spoils only its own
 *   ancestors.  out_valid and out_coverage may be NULL.  The bits depend on neither the tiling nor the number of launches.
 * mi_lightmap_sample_lod / mi_lightmap_sh_sample_lod: the lists of mi_lightmap_sample / mi_lightmap_sh_sample with `levels`, `mips` and
 *   `mip_valid` as mi_lightmap_mips wrote them (both may be NULL when the chain has one level; mip_valid == NULL: every texel of every
 *   level above 0 is valid) and `lod` [n].  Per point: lam = fminf(fmaxf(lod, 0), (float)(L-1)) — a NaN becomes 0 —
 *   l_a = min((int)floorf(lam), max(L-2, 0)), f = lam - (float)l_a, l_b = min(l_a + 1, L-1); the level weights are { 1 - f, f }, and a
 *   level whose weight is not > 0 takes no part and is not read.  Per level l that takes part and per axis g = (t * (float)n_0) * 2^-l
 *   - 0.5f, then the clamp and index expressions of the bilinear form above with n_l; the scaling is exact, and at l = 0 this is the
 *   bilinear form's own expression.  Taps: level a then level b, each dy outer, dx inner; w = w_level * (wx[dx] * wy[dy]); a tap takes
 *   part when w > 0 and its texel is valid at its level.  One acc and one sw over the up to eight taps; out = acc / sw when sw > 0, else
 *   +0.0; out_weight = sw.  The SH form turns each tap's record into e (mi_lightmap_sh_sample's expression) before it is weighted:
 *   three accumulators, never an interpolated record; an all-zero normal gives +0.0 and weight 0.
 *   So with levels == 1, lod <= 0 or a NaN lod the result is mi_lightmap_sample / mi_lightmap_sh_sample of level 0, bit for bit; at an
 *   integer lod = l on a size divisible by 2^l it is mi_lightmap_sample of level l with that level's mip_valid.
 *   Every address is made from clamped indices, whatever uv, lod, the normals and the texels hold.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): a NULL image / sh, out_mips, uv, lod, normals
 *   or out / out_irradiance; mips == NULL with more than one level in the lookups; width or height 0 or above 32768; channels other
 *   than 3 or 27; levels above the full chain; unknown flag bits, and MI_LS_NEAREST in the _lod forms (nearest addressing is the
 *   reference's, and the reference has no mips); in the _device forms an output that overlaps an input.  MI_OK and nothing launched:
 *   mi_lightmap_mips with one level (levels == 1, or a 1 x 1 image), and n == 0.
 * Host forms: HOST pointers, blocking.  _device forms: DEVICE pointers on ctx's device, queued on `stream`, no synchronisation;
 *   mi_last_kernel_ms reports the launches' span.  mi_lightmap_mips_device launches ceil((L-1) / 5) kernels (five levels per launch
 *   from one 32 x 32 tile, staged in LDS; MI_RT_LMM_LEVELS_PER_LAUNCH=1 at context creation: one level per launch, the same bytes).
 *   A later launch reads the coverage of the last level the one before wrote: with out_coverage == NULL the coverage planes live in a
 *   buffer the context owns, so two such calls on one context must not be in flight at once (pass out_coverage to overlap them).  The
 *   lookups need no scratch.  Indices are 64-bit.
 * Out of scope: block-compressed mips are encoded level by level ("BC6H lightmaps" below); deriving lod from ray footprints, anisotropic filtering, wrap modes other than clamp. */
int  mi_lightmap_mips(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                      uint32_t levels, float* out_mips, uint8_t* out_valid, float* out_coverage);
int  mi_lightmap_mips_device(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                             uint32_t levels, float* out_mips, uint8_t* out_valid, float* out_coverage, void* stream);
int  mi_lightmap_sample_lod(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                            uint32_t levels, const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv, const float* lod,
                            uint32_t flags, float* out, float* out_weight);
int  mi_lightmap_sample_lod_device(mi_ctx* ctx, uint32_t width, uint32_t height, uint32_t channels, const float* image, const uint8_t* valid,
                                   uint32_t levels, const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                   const float* lod, uint32_t flags, float* out, float* out_weight, void* stream);
int  mi_lightmap_sh_sample_lod(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t levels,
                               const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv, const float* normals,
                               const float* lod, uint32_t flags, float* out_irradiance, float* out_weight);
int  mi_lightmap_sh_sample_lod_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* sh, const uint8_t* valid, uint32_t levels,
                                      const float* mips, const uint8_t* mip_valid, uint32_t n, const float* uv, const float* normals,
                                      const float* lod, uint32_t flags, float* out_irradiance, float* out_weight, void* stream);

/* ---- packed lightmaps: f16 and RGB9E5 storage and lookups that read them (added within ABI version 5: detect by symbol lookup) ----
 * A finished directional lightmap is 108 bytes per texel in f32.  mi_lightmap_pack stores it (or a plain one, or a mip chain) in one of
 *   two formats that decode to f32 EXACTLY, and mi_lightmap_sample_packed / mi_lightmap_sh_sample_packed read such storage directly.
 *   lightmap_pack, lightmap_unpack, lightmap_sample_packed and lightmap_sh_sample_packed (Python) are the definitions.
 * MI_LP_F16 — channels 3 or 27; a texel is `channels` consecutive u16, tightly packed (6 or 54 bytes: 2-byte aligned only).
 *   Encode per float x: if x != x, the bits are 0x7E00 (made by a select, not by a conversion, so they compare).  Otherwise
 *   c = fminf(fmaxf(x, -65504.0f), 65504.0f), then IEEE round-to-nearest-even f32 -> binary16 of c.  Subnormal results are kept and the
 *   sign of zero is kept.  Infinities and everything beyond +-65504 saturate to 0x7BFF / 0xFBFF: no infinity is ever written.
 *   Decode: the exact binary16 -> f32 widening.
 * MI_LP_RGB9E5 — channels 3 only; a texel is one u32: the shared-exponent format of EXT_texture_shared_exponent / DXGI R9G9B9E5,
 *   N = 9, B = 15, largest value 65408.  The encoder is all f32, with no fused multiply-add.
 *   Per channel: c = (x != x) ? 0 : fminf(fmaxf(x, 0), 65408.0f).  m = max(c_r, c_g, c_b).
 *   eb = ((bits(m) >> 23) & 255) - 127: floor(log2 m) for every m that matters; a zero or subnormal m gives -127.
 *   ep = max(eb, -16) + 16.  ms = floorf(m * 2^(24-ep) + 0.5f).  e = ep + (ms == 512).
 *   q_k = (uint)floorf(c_k * 2^(24-e) + 0.5f).  word = q_r | q_g << 9 | q_b << 18 | e << 27.
 *   The powers of two are exact f32 constants built from the exponent, and the products are exact.  The one rounding per channel is the
 *   + 0.5f, so (0.5 - 2^-25) scaled rounds UP: that is the definition, not a bug.  Decode: (float)q_k * 2^(e-24), exact.
 *   Every q stays <= 511 and every e <= 31; the error per channel is at most 2^(e-25) — half a step; 2^(e-49) more for a channel in
 *   [0.5 - 2^-25, 0.5) steps, the one case where the + 0.5f itself rounds — and at most m / 511 where e > 0.
 *   RGB9E5 at 27 channels is refused, because SH coefficients are signed: directional lightmaps pack as f16.
 * mi_lightmap_pack / mi_lightmap_unpack are layout-agnostic: a count of texels, so level 0 and the `mips` buffer of mi_lightmap_mips
 *   are packed by one call each.  The mip layout, `valid`, `mip_valid` and the coverage planes are unchanged and stay u8 / f32.
 *   Texels behind valid == 0 are encoded like any other and never fault.
 * mi_lightmap_sample_packed / mi_lightmap_sh_sample_packed (the latter MI_LP_F16 only): with lod != NULL the result is, BIT FOR BIT,
 *   mi_lightmap_sample_lod / mi_lightmap_sh_sample_lod on the unpacked level 0 and mips.  With lod == NULL it is mi_lightmap_sample /
 *   mi_lightmap_sh_sample on the unpacked image: then `levels` must be 1 and `mips`, `mip_valid` NULL, and MI_LS_NEAREST is allowed —
 *   with it a texel comes back as it stands: the decoded value, -0.0 included for f16.  All the rules of the two sections above carry
 *   over word for word: tap order, a tap that takes no part is not read, clamped indices only, 64-bit indexing, NaN behaviour,
 *   out_weight.  The lookup arithmetic exists once: the packed kernels are the f32 kernels' device code with another texel fetch.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): everything the f32 calls refuse; an unknown
 *   format or format 0; MI_LP_RGB9E5 with channels other than 3; any format but MI_LP_F16 in the SH form; lod == NULL with levels != 1
 *   or a non-NULL mips / mip_valid; a NULL texels / packed / out_packed / out_texels; n_texels above 2^32; in the _device forms an
 *   output that overlaps an input.  n_texels == 0 / n == 0 is MI_OK and launches nothing.
 * Host forms: HOST pointers, blocking; the arrays pass through the buffer the context owns.  _device forms: DEVICE pointers on ctx's
 *   device, queued on `stream`, no synchronisation, no scratch; mi_last_kernel_ms reports the kernel.
 * Out of scope: lossy block compression here (BC6H has calls of its own: "BC6H lightmaps" below), signed shared-exponent formats, packing `valid` or the coverage planes, packed outputs
 *   of bake, finish or mips (pack is a separate call). */
int  mi_lightmap_pack(mi_ctx* ctx, uint32_t format, uint32_t channels, uint64_t n_texels, const float* texels, void* out_packed);
int  mi_lightmap_pack_device(mi_ctx* ctx, uint32_t format, uint32_t channels, uint64_t n_texels, const float* texels, void* out_packed,
                             void* stream);
int  mi_lightmap_unpack(mi_ctx* ctx, uint32_t format, uint32_t channels, uint64_t n_texels, const void* packed, float* out_texels);
int  mi_lightmap_unpack_device(mi_ctx* ctx, uint32_t format, uint32_t channels, uint64_t n_texels, const void* packed, float* out_texels,
                               void* stream);
int  mi_lightmap_sample_packed(mi_ctx* ctx, uint32_t format, uint32_t width, uint32_t height, uint32_t channels, const void* image,
                               const uint8_t* valid, uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n,
                               const float* uv, const float* lod, uint32_t flags, float* out, float* out_weight);
int  mi_lightmap_sample_packed_device(mi_ctx* ctx, uint32_t format, uint32_t width, uint32_t height, uint32_t channels, const void* image,
                                      const uint8_t* valid, uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n,
                                      const float* uv, const float* lod, uint32_t flags, float* out, float* out_weight, void* stream);
int  mi_lightmap_sh_sample_packed(mi_ctx* ctx, uint32_t format, uint32_t width, uint32_t height, const void* sh, const uint8_t* valid,
                                  uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                  const float* normals, const float* lod, uint32_t flags, float* out_irradiance, float* out_weight);
int  mi_lightmap_sh_sample_packed_device(mi_ctx* ctx, uint32_t format, uint32_t width, uint32_t height, const void* sh,
                                         const uint8_t* valid, uint32_t levels, const void* mips, const uint8_t* mip_valid, uint32_t n,
                                         const float* uv, const float* normals, const float* lod, uint32_t flags, float* out_irradiance,
                                         float* out_weight, void* stream);

/* ---- BC6H lightmaps: a GPU encoder, a decoder and a lookup that reads blocks (added within ABI version 5: detect by symbol lookup) ----
 * BC6H_UF16 (unsigned, 3 channels) is the format in which HDR lightmaps reach a renderer: 16 bytes per 4 x 4 texels, one byte a texel.
 *   It is LOSSY, so it has calls of its own: the MI_LP_* calls above keep their contract ("decodes to f32 exactly") and refuse it.
 *   lightmap_bc6h_encode, lightmap_bc6h_decode, lightmap_bc6h_layout and lightmap_sample_bc6h (Python) are the definitions.
 * ONE block mode is written and read: the one-region mode with two 10-bit direct endpoints and 4-bit indices ("mode 11").  A block is a
 *   little-endian 128-bit integer.  Bits 0-4 hold 3.  Six 10-bit fields follow: rw at bit 5, gw 15, bw 25 (endpoint 0), rx 35, gx 45,
 *   bx 55 (endpoint 1).  From bit 65 texel 0 has a 3-bit index (its top bit is implied 0), texels 1 .. 15 four bits each; texel
 *   t = (y & 3) * 4 + (x & 3).
 * Decode, all integer: unquantise a field q: 0 gives 0, 1023 gives 0xFFFF, else ((q << 16) + 0x8000) >> 10.  With
 *   W = {0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64}: c = (a * (64 - W[i]) + b * W[i] + 32) >> 6, h = (c * 31) >> 6,
 *   and h (at most 0x7BFF) is read as binary16 bits and widened exactly to f32.  A block whose low five bits are not 3 decodes to
 *   sixteen zero texels: other encoders' two-region and delta modes, the other one-region widths and the reserved modes are NOT read
 *   (lightmap_bc6h_modes counts the low five bits of a file's blocks, so a caller can tell).
 * Layout: a level of w x h texels is ceil(w / 4) x ceil(h / 4) blocks, row-major in the image's own row order, 16-byte aligned.  A
 *   chain is level 0 in one buffer and levels 1 .. L - 1 one after the other in a second, the image / mips split of the _lod calls;
 *   the levels' extents are mi_lightmap_mips' (lightmap_mip_layout), the block counts and offsets lightmap_bc6h_layout's.
 * mi_lightmap_bc6h_encode: `image` [height][width][3] f32, `valid` NULL or [height][width], `rounds` 0 .. 4; writes the level's blocks.
 *   One level per call: the caller walks a chain with the layout rule, each level with its own mip_valid.  All integer after step 1:
 *   1. Per texel and channel: c = min(x, 65504) where x > 0, else 0 (a NaN, a negative, -0.0); h = round-to-nearest-even binary16 bits.
 *   2. A texel TAKES PART when it lies inside the image and valid is NULL or non-zero there.  One that does not is not read and never
 *      influences a bit.  A block in which nothing takes part is the word 3 followed by zeros.
 *   3. A texel's error is the squared distance of its h to the block's exact decode, summed over channels (64-bit sums); a block's
 *      error the sum over the texels that take part.  Given endpoints every texel has the index of least error, the lowest on a tie; a
 *      texel that takes no part gets the index best for the integer (floor) mean of the h that take part, so the gutter decodes to
 *      something a hardware filter can touch.
 *   4. Start: the pair (i <= j) of texels that take part farthest apart in h (squared distance), the lowest (i, j) on a tie; endpoint 0
 *      from texel i, endpoint 1 from j.  Per channel c = (64 h + 30) / 31, the smallest c with (c * 31) >> 6 == h, and the field whose
 *      unquantised value is nearest to c, the lower field on a tie.
 *   4b. A flat start: if the two endpoints have the same field in every channel, a channel whose field's unquantised value lies more
 *      than 32 from endpoint 0's c takes the two fields around c instead, (0, 1) where c < 96 and (1022, 1023) otherwise, and the
 *      indices interpolate.  (The unquantised fields are 0, 96, 160, .., 64 q + 32, .., 65440, 65535: only at the two ends can the
 *      nearest be more than 32 away.)  With it a constant block decodes within 16 units of h.
 *   5. `rounds` times: with u = 64 - W[index], v = W[index] over the texels that take part and c as in 4: Suu, Suv, Svv, Suc, Svc the
 *      sums of products, det = Suu Svv - Suv Suv.  Unless det == 0 a channel's endpoints are a = floor((2 na + det) / (2 det)) with
 *      na = 64 (Svv Suc - Suv Svc) and b likewise with nb = 64 (Suu Svc - Suv Suc), clamped to 0 .. 65535 and quantised as in 4.
 *      Indices are assigned again and the result is kept ONLY IF the block's error is strictly lower: the error is monotone in
 *      `rounds`, and a block that already decodes exactly stays as it is.
 *   6. If texel 0's index is 8 or more the endpoints swap and every index i becomes 15 - i (W[15 - i] = 64 - W[i]: the same decode).
 *   (The kernel takes one lane per block; MI_RT_LMB_LANE_PER_BLOCK=0 at context creation selects the kernel that takes a texel per
 *   lane and a block per 16-lane row: the same bytes, slower.)
 * mi_lightmap_bc6h_decode: the level's blocks to [height][width][3] f32.
 * mi_lightmap_sample_bc6h: mi_lightmap_sample_packed's rules word for word, three channels, the texels in blocks: with lod != NULL the
 *   result is, BIT FOR BIT, mi_lightmap_sample_lod on the decoded levels; with lod == NULL mi_lightmap_sample on the decoded image:
 *   then `levels` must be 1 and `mip_blocks`, `mip_valid` NULL, and MI_LS_NEAREST is allowed.  Tap order, a tap that takes no part is
 *   not read (its block is not loaded), clamped indices only, 64-bit indexing, NaN behaviour and out_weight carry over.  `valid` and
 *   `mip_valid` are per TEXEL, in mi_lightmap_mips' layout, as for the f32 calls.
 * MI_ERR_INVALID (each with a message, checked before the context, nothing is launched): everything the f32 lookups refuse; rounds
 *   above 4; a NULL image / blocks / out; in the _device forms blocks that are not 16-byte aligned and an output that overlaps an
 *   input.  n == 0 is MI_OK and launches nothing.
 * Host forms: HOST pointers, blocking; the arrays pass through the buffer the context owns.  _device forms: DEVICE pointers on ctx's
 *   device, queued on `stream`, no synchronisation, no scratch; mi_last_kernel_ms reports the kernel.
 * Out of scope: every other block mode, the signed format (BC6H_SF16), DDS / KTX containers, and 27-channel SH records, which are
 *   signed and stay MI_LP_F16. */
int  mi_lightmap_bc6h_encode(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const uint8_t* valid, uint32_t rounds,
                             void* out_blocks);
int  mi_lightmap_bc6h_encode_device(mi_ctx* ctx, uint32_t width, uint32_t height, const float* image, const uint8_t* valid, uint32_t rounds,
                                    void* out_blocks, void* stream);
int  mi_lightmap_bc6h_decode(mi_ctx* ctx, uint32_t width, uint32_t height, const void* blocks, float* out_image);
int  mi_lightmap_bc6h_decode_device(mi_ctx* ctx, uint32_t width, uint32_t height, const void* blocks, float* out_image, void* stream);
int  mi_lightmap_sample_bc6h(mi_ctx* ctx, uint32_t width, uint32_t height, const void* image_blocks, const uint8_t* valid, uint32_t levels,
                             const void* mip_blocks, const uint8_t* mip_valid, uint32_t n, const float* uv, const float* lod,
                             uint32_t flags, float* out, float* out_weight);
int  mi_lightmap_sample_bc6h_device(mi_ctx* ctx, uint32_t width, uint32_t height, const void* image_blocks, const uint8_t* valid,
                                    uint32_t levels, const void* mip_blocks, const uint8_t* mip_valid, uint32_t n, const float* uv,
                                    const float* lod, uint32_t flags, float* out, float* out_weight, void* stream);

/* Size and allocate the wavefront pipeline's HBM buffers (path state, sample slots) for
 * this camera with the image shared by `world` ranks, so that the first render does not pay the
 * allocation (about 110 GB for a whole 1080p / 256 spp frame on one GPU).  `max_state_bytes` as in
 * mi_render_opts (0 = the frame in one batch, at most 60 % of the free HBM).  Optional. */
int  mi_reserve(mi_ctx* ctx, const mi_camera_desc* cam, int32_t world, uint64_t max_state_bytes);

/* Wavefront pipeline (MI_VARIANT_WAVEFRONT) of the most recent render: out8 = { sum of wf_main
 * launch durations, of wf_trav, of wf_reduce (ms, HIP events around every launch), launches, sum of wf_trav_f, of
 * wf_replay (the two-stage mesh traversal), sum of the spans of wf_main's class-A parts, sum of wf_reduce_sh (mi_render_probes) or of
 * wf_reduce_m2 (mi_render_points_moments, mi_bake_lightmap_moments) or of wf_reduce_psh (mi_render_points_sh, mi_bake_lightmap_sh): no two
 * of them run in one render, and the entry is 0 for every other render }.  A pass after the first launches
 * wf_main in two parts: the class-A blocks run on a second stream BESIDE the walkers of the previous pass (their span includes
 * waiting for CUs the walkers still hold, so it overlaps the wf_trav figure and must not be added to it), the class-B blocks
 * behind the walkers (counted under wf_main). */
int  mi_last_pipeline_ms(mi_ctx* ctx, float* out8);

/* Path counts of the most recent wavefront render, for traffic accounting: out8 = { passes (wf_main launches
 * that left survivors or ended the batch), class-A paths written to (and read back from) the HBM path state summed
 * over the passes, class-B paths likewise, slots the mesh walkers went through (= the class-B paths: the walkers read those lists, there is no queue), sample slots, compact pixels,
 * path segments (every Scene::intersect_ray evaluation, tracing.rs:305, counted on the device by wf_main), samples of dead tiles (tiles from which
 * no camera ray can reach anything: no ray is generated for them — they are black by tracing.rs:306 — and none of the other counts includes them;
 * 0 when signatures were asked for) }.
 * The bytes these stand for (72 B per class-A path and direction, 76 B per class-B path, ...) are in DESIGN.md. */
int  mi_last_pipeline_counts(mi_ctx* ctx, uint64_t* out8);

/* Counters of the most recent *_DIAG launch (synchronises the device):
 * out16 = { A trips, sum of lanes in A trips, interior-step trips, lanes, leaf-step trips,
 *           lanes, B trips, waves, shader-clock cycles in A trips, in B trips, cycles in A's
 *           shade / regenerate / list sections, slab tests inside trees, path segments, 0 }.
 * active-lane fraction of a phase = lanes / (64 * trips). */
int  mi_last_diag(mi_ctx* ctx, uint64_t* out16);

/* Self-test of the kernels' arithmetic shortcuts on this device (about a second).  The kernels compute `1.0 / x` — the
 * reference's Moller-Trumbore `f = 1.0/a` (geometry.rs:340,437), `inv_d` (geometry.rs:57), cgmath's normalize — with a
 * 5-instruction sequence (v_rcp_f32 + one fused Newton step, IEEE division outside the exponent range where that is proven)
 * instead of the 11-instruction IEEE division; this sweeps ALL 2^32 f32 bit patterns and counts the inputs for which the
 * two differ in any bit.  out4 = { mismatches (must be 0), inputs checked, 0, 0 }. */
int  mi_selftest(mi_ctx* ctx, uint64_t* out4);

/* ---- multi-GPU behind the ABI: replaces rayon's row split (tracing.rs:228) with N devices of one node ----
 * One mi_multi owns one context, stream and (per frame) one host thread per device.  The image is cut into MI_TILE^2 tiles,
 * tile t rendered on device t % N; per frame there is exactly ONE exchange — every peer sends its compact tile buffer to
 * device 0 over its own xGMI link (RCCL ncclSend / ncclRecv in one group, resolved with dlopen at mi_multi_create) — then the
 * un-permute and the tone-map run on device 0 — always, so a call with all three output pointers NULL leaves the finished
 * f32 and u8 images resident on device 0 and moves nothing over PCIe.  The image is bit-identical for every N (the RNG is
 * keyed by the global pixel index).  `devices` = NULL means 0 .. n_devices-1.  mi_multi_render: as mi_render; opts->rank / world are ignored;
 * stats->kernel_ms is the slowest device's pipeline pass, stats->total_ms the wall time of the call. */
typedef struct mi_multi mi_multi;
int  mi_multi_create(int n_devices, const int* devices, mi_multi** out);
/* TEST TRANSPORT, not for production use: `n_contexts` ranks that all live on the ONE device `device`, so that everything
 * mi_multi_render does for N >= 2 — one host thread per rank, every rank's pipeline on its own streams, the r * slice receive
 * offsets, the un-permute and tone-map with world > 1, the max-over-ranks statistics — runs on a one-GPU machine.  The only
 * difference from mi_multi_create is the exchange: RCCL is not loaded, and each ncclSend / ncclRecv pair becomes one
 * device-to-device hipMemcpyAsync on the sender's stream that device 0's stream waits for through an event (the ordering
 * the RCCL pair gives).  The ranks share the card, so the call is no faster than mi_render; the image is bit-identical to it.
 * With opts->max_state_bytes == 0 the ranks split the default budget (60 % of the free HBM) evenly. */
int  mi_multi_create_loopback(int n_contexts, int device, mi_multi** out);
void mi_multi_destroy(mi_multi* m);
int  mi_multi_device_count(const mi_multi* m);
/* The context of device number `rank` (0 .. N-1), owned by `m` and valid until mi_multi_destroy: for the per-device queries
 * (mi_last_kernel_ms, mi_last_pipeline_ms, mi_last_pipeline_counts) after a mi_multi_render.  NULL if out of range. */
mi_ctx* mi_multi_context(const mi_multi* m, int rank);
int  mi_multi_scene_upload(mi_multi* m, const mi_scene_desc* scene);
int  mi_multi_reserve(mi_multi* m, const mi_camera_desc* cam, uint64_t max_state_bytes);
int  mi_multi_render(mi_multi* m, const mi_camera_desc* cam, const mi_render_opts* opts,
                     float* out_rgb_f32, uint8_t* out_rgb_u8, uint32_t* out_sig, mi_stats* stats);

/* Thread-local message of the most recent failure in this thread. */
const char* mi_last_error(void);
int  mi_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MI_RT_H */
