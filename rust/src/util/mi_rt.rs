//! Rust binding of include/mi_rt.h for mbk6/CS397RayTracingSP22: what a maintainer of the reference adds as
//! `src/util/mi_rt.rs` (rust/README.md lists the other files of the patch set and the five lines of the reference they touch).
//! UNVERIFIED BY A COMPILER IN THIS CONTAINER: there is no cargo / rustc here.  What IS checked mechanically
//! (tests/test_abi.py): every `#[repr(C)]` struct below against the C header field by field (order, type, count), every
//! `extern "C"` function against the header's prototypes (name, argument count and types), the numeric constants, and the
//! bracket structure of every file of the patch set.
#![allow(non_camel_case_types, dead_code)]
use std::collections::HashMap;
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] #[derive(Clone, Copy)] pub struct mi_material { pub kind: i32, pub albedo: [f32; 3], pub emission: [f32; 3], pub roughness: f32, pub metallic: f32, pub idx_of_refraction: f32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_object { pub kind: i32, pub index: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_sphere { pub center: [f32; 3], pub radius: f32, pub material: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_triangle { pub a: [f32; 3], pub b: [f32; 3], pub c: [f32; 3], pub material: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_plane { pub point: [f32; 3], pub normal: [f32; 3], pub material: i32 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_volume { pub boundary_center: [f32; 3], pub boundary_radius: f32, pub density: f32, pub phase_material: i32,
    pub boundary_kind: i32, pub boundary_index: i32, pub boundary_count: i32 }   // 0 = the inline sphere; else Triangle / Plane / StaticMesh / nested Scene
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_texture { pub width: i32, pub height: i32, pub rgb: *const u8 }
#[repr(C)] #[derive(Clone, Copy)] pub struct mi_mesh {
    pub positions: *const f32, pub normals: *const f32, pub texcoords: *const f32, pub indices: *const u32,
    pub n_vertices: i32, pub n_triangles: i32, pub transform: [f32; 16], pub inv_transform: [f32; 16],
    pub material: i32, pub textures: [i32; 5],
}
#[repr(C)] pub struct mi_scene_desc {
    pub objects: *const mi_object, pub n_objects: i32, pub spheres: *const mi_sphere, pub n_spheres: i32,
    pub triangles: *const mi_triangle, pub n_triangles: i32, pub planes: *const mi_plane, pub n_planes: i32,
    pub volumes: *const mi_volume, pub n_volumes: i32, pub meshes: *const mi_mesh, pub n_meshes: i32,
    pub materials: *const mi_material, pub n_materials: i32, pub textures: *const mi_texture, pub n_textures: i32,
    pub boundary_objects: *const mi_object, pub n_boundary_objects: i32,   // entries of nested Scenes used as ConvexVolume boundaries
    pub point_light_pos: [f32; 3], pub ambient: [f32; 3],   // Scene.point_light_pos / ambient (tracing.rs:216-217), Phong only
}
#[repr(C)] pub struct mi_camera_desc {
    pub eyepoint: [f32; 3], pub view_dir: [f32; 3], pub up: [f32; 3], pub projection_mode: i32, pub shading_mode: i32,
    pub path_depth: u32, pub path_samples: u32, pub screen_width: u32, pub screen_height: u32,
    pub focal_length: f32, pub focus_dist: f32, pub lens_radius: f32, pub aa_sample_count: u32, pub max_trace_dist: f32, pub gamma: f32,
}
#[repr(C)] #[derive(Default)] pub struct mi_render_opts { pub seed: u32, pub rank: i32, pub world: i32, pub variant: i32, pub want_signature: i32, pub flags: u32, pub max_state_bytes: u64 }
#[repr(C)] #[derive(Default)] pub struct mi_stats { pub samples: u64, pub pixels: u64, pub tiles: u32, pub tiles_padded: u32, pub kernel_ms: f32, pub total_ms: f32, pub scene_bytes: u32, pub scene_in_lds: u32 }
// A probe grid for mi_probe_volume_sample (sh and valid: host addresses for the host form, device addresses for the _device form).  The C
// layout, 56 bytes; align(8) spells out the alignment its pointers give it.  tests/test_probe_volume_host.py compares it with the header.
#[repr(C, align(8))] #[derive(Clone, Copy)] pub struct mi_probe_volume {
    pub lo: [f32; 3], pub hi: [f32; 3], pub counts: [u32; 3], pub flags: u32, pub sh: *const f32, pub valid: *const u8,
}
// The parameters of mi_bake_lightmap_adaptive.  The C layout, 20 bytes; align(4) spells out the alignment its fields give it.
#[repr(C, align(4))] #[derive(Clone, Copy)] pub struct mi_lightmap_adaptive {
    pub first_samples: u32, pub round_samples: u32, pub max_rounds: u32, pub target_rel: f32, pub target_abs: f32,
}
pub enum mi_ctx {}
pub enum mi_multi {}
pub const MI_OPT_NO_TILE_MASKS: u32 = 1; pub const MI_OPT_REFERENCE_WALK: u32 = 2; pub const MI_OPT_TWO_STAGE: u32 = 4; pub const MI_OPT_NO_LIST_TREE: u32 = 8; pub const MI_OPT_NO_FINAL_CULL: u32 = 16;
pub const MI_RT_ABI_VERSION: c_int = 5;
pub const MI_HEMI_WORLD_RADIUS: u32 = 1;
pub const MI_LM_JITTER: u32 = 1;
pub const MI_PV_NORMAL_WEIGHT: u32 = 1;
pub const MI_LS_NEAREST: u32 = 1;
pub const MI_LP_F16: u32 = 1;
pub const MI_LP_RGB9E5: u32 = 2;
pub const MI_BC6H_BLOCK_BYTES: u32 = 16;
pub const MI_BC6H_BLOCK_DIM: u32 = 4;
pub const MI_BC6H_MODE: u32 = 3;
pub const MI_BC6H_MAX_ROUNDS: u32 = 4;
// mi_material_kind / mi_object_kind / projection and shading modes (include/mi_rt.h)
pub const MI_MAT_LAMBERTIAN: i32 = 0; pub const MI_MAT_METAL: i32 = 1; pub const MI_MAT_DIELECTRIC: i32 = 2;
pub const MI_MAT_PARAMETERIZED: i32 = 3; pub const MI_MAT_ISOTROPIC: i32 = 4;
pub const MI_OBJ_SPHERE: i32 = 0; pub const MI_OBJ_TRIANGLE: i32 = 1; pub const MI_OBJ_PLANE: i32 = 2;
pub const MI_OBJ_VOLUME: i32 = 3; pub const MI_OBJ_MESH: i32 = 4; pub const MI_OBJ_SCENE: i32 = 5;
pub const MI_PROJ_ORTHOGRAPHIC: i32 = 0; pub const MI_PROJ_PERSPECTIVE: i32 = 1;
pub const MI_SHADE_PHONG: i32 = 0; pub const MI_SHADE_PATHTRACE: i32 = 1;

#[link(name = "mi_rt")]
extern "C" {
    // every entry point of include/mi_rt.h (ABI 5), in header order
    pub fn mi_ctx_create(device: c_int, out: *mut *mut mi_ctx) -> c_int;
    pub fn mi_ctx_destroy(ctx: *mut mi_ctx);
    pub fn mi_scene_upload(ctx: *mut mi_ctx, scene: *const mi_scene_desc) -> c_int;
    pub fn mi_render(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                     out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_compact_size(cam: *const mi_camera_desc, world: i32, tiles_total: *mut u32, tiles_padded: *mut u32) -> c_int;
    // device-pointer building blocks (one process per GPU); pointers are device addresses, `stream` a hipStream_t
    pub fn mi_render_tiles_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                  d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_samples_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                    sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void,
                                    d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    pub fn mi_unpermute_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, world: i32,
                               d_gathered_f32: *const c_void, d_image_f32: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn mi_tonemap_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, d_image_f32: *const c_void, d_image_u8: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn mi_last_kernel_ms(ctx: *mut mi_ctx, ms: *mut f32) -> c_int;
    // ray queries (added within ABI 5; a caller that may meet an older library looks the symbols up)
    pub fn mi_intersect_rays(ctx: *mut mi_ctx, n_rays: u32, origins: *const f32, dirs: *const f32, t_min: f32, t_max: f32,
                             seed: u32, first_key: u32, out_object: *mut i32, out_distance: *mut f32, out_hitpoint: *mut f32,
                             out_normal: *mut f32, out_flags: *mut i32, out_uv: *mut f32, out_material: *mut mi_material) -> c_int;
    pub fn mi_intersect_rays_device(ctx: *mut mi_ctx, n_rays: u32, origins: *const f32, dirs: *const f32, t_min: f32, t_max: f32,
                                    seed: u32, first_key: u32, out_object: *mut i32, out_distance: *mut f32, out_hitpoint: *mut f32,
                                    out_normal: *mut f32, out_flags: *mut i32, out_uv: *mut f32, out_material: *mut mi_material,
                                    stream: *mut c_void) -> c_int;
    pub fn mi_shade_rays(ctx: *mut mi_ctx, cam: *const mi_camera_desc, n_rays: u32, origins: *const f32, dirs: *const f32,
                         seed: u32, first_key: u32, out_rgb: *mut f32) -> c_int;
    pub fn mi_shade_rays_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, n_rays: u32, origins: *const f32, dirs: *const f32,
                                seed: u32, first_key: u32, out_rgb: *mut f32, stream: *mut c_void) -> c_int;
    // occlusion queries (any-hit; added within ABI 5 like the ray queries).  ray_t_max: null, or one t_max per ray
    pub fn mi_occluded_rays(ctx: *mut mi_ctx, n_rays: u32, origins: *const f32, dirs: *const f32, t_min: f32, t_max: f32,
                            ray_t_max: *const f32, seed: u32, first_key: u32, out_occluded: *mut u8) -> c_int;
    pub fn mi_occluded_rays_device(ctx: *mut mi_ctx, n_rays: u32, origins: *const f32, dirs: *const f32, t_min: f32, t_max: f32,
                                   ray_t_max: *const f32, seed: u32, first_key: u32, out_occluded: *mut u8, stream: *mut c_void) -> c_int;
    pub fn mi_hemisphere_occlusion(ctx: *mut mi_ctx, n_points: u32, points: *const f32, normals: *const f32, first_sample: u32,
                                   n_samples: u32, t_min: f32, t_max: f32, flags: u32, seed: u32, first_key: u32,
                                   out_open: *mut u32, out_bent: *mut f32) -> c_int;
    pub fn mi_hemisphere_occlusion_device(ctx: *mut mi_ctx, n_points: u32, points: *const f32, normals: *const f32, first_sample: u32,
                                          n_samples: u32, t_min: f32, t_max: f32, flags: u32, seed: u32, first_key: u32,
                                          out_open: *mut u32, out_bent: *mut f32, stream: *mut c_void) -> c_int;
    // ray-table rendering (added within ABI 5): origins / dirs are [rays_per_pixel][H][W][3], rays_per_pixel = 1 or aa_sample_count
    pub fn mi_render_rays(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                          origins: *const f32, dirs: *const f32, rays_per_pixel: u32,
                          out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_rays_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                 d_origins: *const f32, d_dirs: *const f32, rays_per_pixel: u32,
                                 sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void,
                                 d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    // point-table rendering (added within ABI 5): points / normals are [rows_per_pixel][H][W][3]; the directions are drawn on the GPU
    pub fn mi_render_points(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                            points: *const f32, normals: *const f32, rows_per_pixel: u32,
                            out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_points_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                   d_points: *const f32, d_normals: *const f32, rows_per_pixel: u32,
                                   sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void,
                                   d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    // lightmap atlas (added within ABI 5): the point table of a mesh's uv atlas made on the GPU, [rows][H][W][3] / [rows][H][W]
    pub fn mi_lightmap_texels(ctx: *mut mi_ctx, mesh: *const mi_mesh, width: u32, height: u32, rows: u32, flags: u32,
                              seed: u32, offset: f32, out_points: *mut f32, out_normals: *mut f32, out_triangle: *mut i32) -> c_int;
    pub fn mi_lightmap_texels_device(ctx: *mut mi_ctx, mesh: *const mi_mesh, width: u32, height: u32, rows: u32, flags: u32,
                                     seed: u32, offset: f32, out_points: *mut f32, out_normals: *mut f32, out_triangle: *mut i32,
                                     stream: *mut c_void) -> c_int;
    pub fn mi_bake_lightmap(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts, mesh: *const mi_mesh, flags: u32,
                            offset: f32, out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, out_triangle: *mut i32,
                            stats: *mut mi_stats) -> c_int;
    // lightmap finishing (added within ABI 5): edge-aware a-trous filter and gutter dilation; image / points / normals / out_image are
    // [H][W][3], out_valid [H][W] bytes or null
    pub fn mi_lightmap_finish(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, points: *const f32, normals: *const f32,
                              levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                              dilate: u32, out_image: *mut f32, out_valid: *mut u8) -> c_int;
    pub fn mi_lightmap_finish_device(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, points: *const f32, normals: *const f32,
                                     levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                                     dilate: u32, out_image: *mut f32, out_valid: *mut u8, stream: *mut c_void) -> c_int;
    // lightmap variance (added within ABI 5): the bake's second moments, out_m2 [H][W][3] / d_compact_m2 [tiles_padded][1024][3], and the
    // finish they guide (m2 and samples behind the image, color_floor behind sigma_color, out_var [H][W] or null behind out_image)
    pub fn mi_render_points_moments(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                    points: *const f32, normals: *const f32, rows_per_pixel: u32, out_m2: *mut f32,
                                    out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_points_moments_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                           d_points: *const f32, d_normals: *const f32, rows_per_pixel: u32,
                                           sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void, d_compact_m2: *mut c_void,
                                           d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    pub fn mi_bake_lightmap_moments(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts, mesh: *const mi_mesh, flags: u32,
                                    offset: f32, out_m2: *mut f32, out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32,
                                    out_triangle: *mut i32, stats: *mut mi_stats) -> c_int;
    pub fn mi_lightmap_finish_var(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32, samples: u32,
                                  points: *const f32, normals: *const f32, levels: u32, normal_power_log2: u32, sigma_plane: f32,
                                  reach: f32, sigma_color: f32, color_floor: f32, dilate: u32, out_image: *mut f32, out_var: *mut f32,
                                  out_valid: *mut u8) -> c_int;
    pub fn mi_lightmap_finish_var_device(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32, samples: u32,
                                         points: *const f32, normals: *const f32, levels: u32, normal_power_log2: u32,
                                         sigma_plane: f32, reach: f32, sigma_color: f32, color_floor: f32, dilate: u32, out_image: *mut f32,
                                         out_var: *mut f32, out_valid: *mut u8, stream: *mut c_void) -> c_int;
    // adaptive lightmap bake (added within ABI 5): the texels whose variance asks for more samples (ascending texel numbers, their count,
    // the error plane or null), their compact point tables [rows][ceil(n / cw)][cw][3], the merge of a round into the running planes, the
    // variance-guided finish with per-texel counts, and the bake that composes them with mi_render_points_moments
    pub fn mi_lightmap_select(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32, counts: *const u32,
                              normals: *const f32, target_rel: f32, target_abs: f32, capacity: u32, out_index: *mut u32,
                              out_count: *mut u32, out_error: *mut f32) -> c_int;
    pub fn mi_lightmap_select_device(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32, counts: *const u32,
                                     normals: *const f32, target_rel: f32, target_abs: f32, capacity: u32, out_index: *mut u32,
                                     out_count: *mut u32, out_error: *mut f32, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_gather(ctx: *mut mi_ctx, width: u32, height: u32, rows: u32, n: u32, index: *const u32,
                              points: *const f32, normals: *const f32, cw: u32, out_points: *mut f32, out_normals: *mut f32) -> c_int;
    pub fn mi_lightmap_gather_device(ctx: *mut mi_ctx, width: u32, height: u32, rows: u32, n: u32, index: *const u32,
                                     points: *const f32, normals: *const f32, cw: u32, out_points: *mut f32, out_normals: *mut f32,
                                     stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_merge(ctx: *mut mi_ctx, width: u32, height: u32, n: u32, index: *const u32, mean: *const f32,
                             m2_round: *const f32, round_samples: u32, image: *mut f32, m2: *mut f32, counts: *mut u32) -> c_int;
    pub fn mi_lightmap_merge_device(ctx: *mut mi_ctx, width: u32, height: u32, n: u32, index: *const u32, mean: *const f32,
                                    m2_round: *const f32, round_samples: u32, image: *mut f32, m2: *mut f32, counts: *mut u32,
                                    stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_finish_var_counts(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32,
                                         counts: *const u32, points: *const f32, normals: *const f32, levels: u32,
                                         normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32, color_floor: f32,
                                         dilate: u32, out_image: *mut f32, out_var: *mut f32, out_valid: *mut u8) -> c_int;
    pub fn mi_lightmap_finish_var_counts_device(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, m2: *const f32,
                                                counts: *const u32, points: *const f32, normals: *const f32, levels: u32,
                                                normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32, color_floor: f32,
                                                dilate: u32, out_image: *mut f32, out_var: *mut f32, out_valid: *mut u8,
                                                stream: *mut c_void) -> c_int;
    pub fn mi_bake_lightmap_adaptive(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts, mesh: *const mi_mesh, flags: u32,
                                     offset: f32, adaptive: *const mi_lightmap_adaptive, out_counts: *mut u32, out_m2: *mut f32,
                                     out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, out_triangle: *mut i32,
                                     stats: *mut mi_stats) -> c_int;
    // light probes (added within ABI 5): points is [rows_per_pixel][H][W][3]; out_sh [H][W][9][3], d_compact_sh [tiles_padded][1024][27]
    pub fn mi_render_probes(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                            points: *const f32, rows_per_pixel: u32, out_sh: *mut f32,
                            out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_probes_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                   d_points: *const f32, rows_per_pixel: u32,
                                   sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void, d_compact_sh: *mut c_void,
                                   d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    // irradiance volumes (added within ABI 5): SH L2 probe grids sampled at surface points; points / normals / out_irradiance are [n][3],
    // out_weight [n] or null; the _device form takes device addresses (in the struct too)
    pub fn mi_probe_volume_sample(ctx: *mut mi_ctx, volume: *const mi_probe_volume, n_points: u32, points: *const f32, normals: *const f32,
                                  out_irradiance: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_probe_volume_sample_device(ctx: *mut mi_ctx, volume: *const mi_probe_volume, n_points: u32, points: *const f32,
                                         normals: *const f32, out_irradiance: *mut f32, out_weight: *mut f32, stream: *mut c_void) -> c_int;
    // directional lightmaps (added within ABI 5): the point-table bake with out_sh [H][W][9][3] / d_compact_sh [tiles_padded][1024][27],
    // mi_lightmap_finish for such records, and the irradiance of n records [n][9][3] at n normals [n][3]
    pub fn mi_render_points_sh(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                               points: *const f32, normals: *const f32, rows_per_pixel: u32, out_sh: *mut f32,
                               out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_render_points_sh_device(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                                      d_points: *const f32, d_normals: *const f32, rows_per_pixel: u32,
                                      sample_begin: u32, sample_end: u32, d_accum_f32x4: *mut c_void, d_compact_sh: *mut c_void,
                                      d_compact_f32: *mut c_void, d_sig_u32: *mut c_void, stream: *mut c_void, stats: *mut mi_stats) -> c_int;
    pub fn mi_bake_lightmap_sh(ctx: *mut mi_ctx, cam: *const mi_camera_desc, opts: *const mi_render_opts, mesh: *const mi_mesh, flags: u32,
                               offset: f32, out_sh: *mut f32, out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32,
                               out_triangle: *mut i32, stats: *mut mi_stats) -> c_int;
    pub fn mi_lightmap_finish_sh(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, points: *const f32, normals: *const f32,
                                 levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                                 dilate: u32, out_sh: *mut f32, out_valid: *mut u8) -> c_int;
    pub fn mi_lightmap_finish_sh_device(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, points: *const f32, normals: *const f32,
                                        levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                                        dilate: u32, out_sh: *mut f32, out_valid: *mut u8, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sh_eval(ctx: *mut mi_ctx, n: u32, sh: *const f32, normals: *const f32, out_irradiance: *mut f32) -> c_int;
    pub fn mi_lightmap_sh_eval_device(ctx: *mut mi_ctx, n: u32, sh: *const f32, normals: *const f32, out_irradiance: *mut f32,
                                      stream: *mut c_void) -> c_int;
    // lightmap lookup: a finished lightmap read at uv points (bilinear over the valid texels, or MI_LS_NEAREST)
    pub fn mi_lightmap_sample(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                              n: u32, uv: *const f32, flags: u32, out: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sample_device(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                                     n: u32, uv: *const f32, flags: u32, out: *mut f32, out_weight: *mut f32, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sh_sample(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, valid: *const u8, n: u32,
                                 uv: *const f32, normals: *const f32, flags: u32, out_irradiance: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sh_sample_device(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, valid: *const u8, n: u32,
                                        uv: *const f32, normals: *const f32, flags: u32, out_irradiance: *mut f32, out_weight: *mut f32,
                                        stream: *mut c_void) -> c_int;
    // lightmap mips: the coverage-aware pyramid (levels 1 .. L - 1, tightly packed) and the trilinear lookups that read it
    pub fn mi_lightmap_mips(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                            levels: u32, out_mips: *mut f32, out_valid: *mut u8, out_coverage: *mut f32) -> c_int;
    pub fn mi_lightmap_mips_device(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                                   levels: u32, out_mips: *mut f32, out_valid: *mut u8, out_coverage: *mut f32, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sample_lod(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                                  levels: u32, mips: *const f32, mip_valid: *const u8, n: u32, uv: *const f32, lod: *const f32,
                                  flags: u32, out: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sample_lod_device(ctx: *mut mi_ctx, width: u32, height: u32, channels: u32, image: *const f32, valid: *const u8,
                                         levels: u32, mips: *const f32, mip_valid: *const u8, n: u32, uv: *const f32, lod: *const f32,
                                         flags: u32, out: *mut f32, out_weight: *mut f32, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sh_sample_lod(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, valid: *const u8, levels: u32,
                                     mips: *const f32, mip_valid: *const u8, n: u32, uv: *const f32, normals: *const f32,
                                     lod: *const f32, flags: u32, out_irradiance: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sh_sample_lod_device(ctx: *mut mi_ctx, width: u32, height: u32, sh: *const f32, valid: *const u8, levels: u32,
                                            mips: *const f32, mip_valid: *const u8, n: u32, uv: *const f32, normals: *const f32,
                                            lod: *const f32, flags: u32, out_irradiance: *mut f32, out_weight: *mut f32,
                                            stream: *mut c_void) -> c_int;
    // packed lightmaps: f16 / RGB9E5 storage (MI_LP_*) and the lookups that read it; lod null = the level-0 lookup
    pub fn mi_lightmap_pack(ctx: *mut mi_ctx, format: u32, channels: u32, n_texels: u64, texels: *const f32, out_packed: *mut c_void) -> c_int;
    pub fn mi_lightmap_pack_device(ctx: *mut mi_ctx, format: u32, channels: u32, n_texels: u64, texels: *const f32, out_packed: *mut c_void,
                                   stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_unpack(ctx: *mut mi_ctx, format: u32, channels: u32, n_texels: u64, packed: *const c_void, out_texels: *mut f32) -> c_int;
    pub fn mi_lightmap_unpack_device(ctx: *mut mi_ctx, format: u32, channels: u32, n_texels: u64, packed: *const c_void, out_texels: *mut f32,
                                     stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sample_packed(ctx: *mut mi_ctx, format: u32, width: u32, height: u32, channels: u32, image: *const c_void,
                                     valid: *const u8, levels: u32, mips: *const c_void, mip_valid: *const u8, n: u32, uv: *const f32,
                                     lod: *const f32, flags: u32, out: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sample_packed_device(ctx: *mut mi_ctx, format: u32, width: u32, height: u32, channels: u32, image: *const c_void,
                                            valid: *const u8, levels: u32, mips: *const c_void, mip_valid: *const u8, n: u32,
                                            uv: *const f32, lod: *const f32, flags: u32, out: *mut f32, out_weight: *mut f32,
                                            stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sh_sample_packed(ctx: *mut mi_ctx, format: u32, width: u32, height: u32, sh: *const c_void, valid: *const u8,
                                        levels: u32, mips: *const c_void, mip_valid: *const u8, n: u32, uv: *const f32,
                                        normals: *const f32, lod: *const f32, flags: u32, out_irradiance: *mut f32,
                                        out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sh_sample_packed_device(ctx: *mut mi_ctx, format: u32, width: u32, height: u32, sh: *const c_void, valid: *const u8,
                                               levels: u32, mips: *const c_void, mip_valid: *const u8, n: u32, uv: *const f32,
                                               normals: *const f32, lod: *const f32, flags: u32, out_irradiance: *mut f32,
                                               out_weight: *mut f32, stream: *mut c_void) -> c_int;
    // BC6H lightmaps: one level per encode / decode call; the lookup reads blocks (lod null = the level-0 lookup)
    pub fn mi_lightmap_bc6h_encode(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, valid: *const u8, rounds: u32,
                                   out_blocks: *mut c_void) -> c_int;
    pub fn mi_lightmap_bc6h_encode_device(ctx: *mut mi_ctx, width: u32, height: u32, image: *const f32, valid: *const u8, rounds: u32,
                                          out_blocks: *mut c_void, stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_bc6h_decode(ctx: *mut mi_ctx, width: u32, height: u32, blocks: *const c_void, out_image: *mut f32) -> c_int;
    pub fn mi_lightmap_bc6h_decode_device(ctx: *mut mi_ctx, width: u32, height: u32, blocks: *const c_void, out_image: *mut f32,
                                          stream: *mut c_void) -> c_int;
    pub fn mi_lightmap_sample_bc6h(ctx: *mut mi_ctx, width: u32, height: u32, image_blocks: *const c_void, valid: *const u8, levels: u32,
                                   mip_blocks: *const c_void, mip_valid: *const u8, n: u32, uv: *const f32, lod: *const f32, flags: u32,
                                   out: *mut f32, out_weight: *mut f32) -> c_int;
    pub fn mi_lightmap_sample_bc6h_device(ctx: *mut mi_ctx, width: u32, height: u32, image_blocks: *const c_void, valid: *const u8,
                                          levels: u32, mip_blocks: *const c_void, mip_valid: *const u8, n: u32, uv: *const f32,
                                          lod: *const f32, flags: u32, out: *mut f32, out_weight: *mut f32, stream: *mut c_void) -> c_int;
    pub fn mi_reserve(ctx: *mut mi_ctx, cam: *const mi_camera_desc, world: i32, max_state_bytes: u64) -> c_int;
    pub fn mi_last_pipeline_ms(ctx: *mut mi_ctx, out8: *mut f32) -> c_int;
    pub fn mi_last_pipeline_counts(ctx: *mut mi_ctx, out8: *mut u64) -> c_int;
    pub fn mi_last_diag(ctx: *mut mi_ctx, out16: *mut u64) -> c_int;
    pub fn mi_selftest(ctx: *mut mi_ctx, out4: *mut u64) -> c_int;
    // N GPUs of one node behind one blocking call (RCCL fan-in inside the library)
    pub fn mi_multi_create(n_devices: c_int, devices: *const c_int, out: *mut *mut mi_multi) -> c_int;
    pub fn mi_multi_create_loopback(n_contexts: c_int, device: c_int, out: *mut *mut mi_multi) -> c_int;   // test transport: N ranks on one device
    pub fn mi_multi_destroy(m: *mut mi_multi);
    pub fn mi_multi_device_count(m: *const mi_multi) -> c_int;
    pub fn mi_multi_context(m: *const mi_multi, rank: c_int) -> *mut mi_ctx;
    pub fn mi_multi_scene_upload(m: *mut mi_multi, scene: *const mi_scene_desc) -> c_int;
    pub fn mi_multi_reserve(m: *mut mi_multi, cam: *const mi_camera_desc, max_state_bytes: u64) -> c_int;
    pub fn mi_multi_render(m: *mut mi_multi, cam: *const mi_camera_desc, opts: *const mi_render_opts,
                           out_rgb_f32: *mut f32, out_rgb_u8: *mut u8, out_sig: *mut u32, stats: *mut mi_stats) -> c_int;
    pub fn mi_last_error() -> *const c_char;
    pub fn mi_abi_version() -> c_int;           // 5: assert at start-up that header and library agree
}


/// The additive half of `trait Intersectable` (tracing.rs:42-47): `pub trait Intersectable: mi_rt::FlattenObject`.
/// A supertrait rather than a new method, so that the implementations live in their own `impl` blocks (the
/// `*_flatten.rs` fragments) and no existing `impl Intersectable for ..` block of the reference is edited.
/// The default body is what the helper types get that never appear in `Scene.objects` (AABB, BVHNode, IndexedTriangle).
pub trait FlattenObject {
    fn flatten(&self, out: &mut SceneBuilder) { out.unsupported(std::any::type_name::<Self>()); }
}
/// The additive half of `trait Material` (materials.rs:12-15): `pub trait Material: mi_rt::FlattenMaterial`.
pub trait FlattenMaterial {
    fn flatten(&self) -> mi_material;
}

/// Collects the PODs of a scene in `Scene.objects` order (that order decides ties, tracing.rs:335, and the order of the
/// RNG draws of ConvexVolume::intersect_ray, geometry.rs:517).  Owns what the PODs point into where the reference does not:
/// the RGB8 bytes of the textures.  Mesh arrays are borrowed from the `Arc<Mesh>` of the StaticMesh, which outlives the call.
#[derive(Default)]
pub struct SceneBuilder {
    pub objects: Vec<mi_object>, pub spheres: Vec<mi_sphere>, pub triangles: Vec<mi_triangle>, pub planes: Vec<mi_plane>,
    pub volumes: Vec<mi_volume>, pub meshes: Vec<mi_mesh>, pub materials: Vec<mi_material>, pub textures: Vec<mi_texture>,
    pub boundary_objects: Vec<mi_object>,
    /// first reason why this scene cannot run on the GPU path (None = it can)
    pub unsupported: Option<String>,
    tex_bytes: Vec<Vec<u8>>,                   // backing store of `textures[i].rgb` (a Vec's heap block does not move when the outer Vec grows)
    material_ids: HashMap<usize, i32>,         // Arc<dyn Material> data pointer -> index: a shared Arc is one mi_material
    mesh_ids: HashMap<usize, i32>,             // &StaticMesh address -> index: the same Arc<StaticMesh> listed twice is ONE mi_mesh
    detached: Vec<Vec<mi_object>>,             // open ConvexVolume boundaries: entries pushed meanwhile are NOT Scene.objects entries
}
impl SceneBuilder {
    pub fn unsupported(&mut self, what: &str) {
        if self.unsupported.is_none() { self.unsupported = Some(what.to_string()); }
    }
    /// One entry of Scene.objects — or, inside a ConvexVolume boundary, one entry of that boundary.
    pub fn push_object(&mut self, kind: i32, index: i32) {
        let o = mi_object { kind: kind, index: index };
        match self.detached.last_mut() { Some(list) => list.push(o), None => self.objects.push(o) }
    }
    pub fn in_boundary(&self) -> bool { !self.detached.is_empty() }
    pub fn begin_boundary(&mut self) { self.detached.push(Vec::new()); }
    pub fn end_boundary(&mut self) -> Vec<mi_object> { self.detached.pop().unwrap_or_default() }
    /// Index of `m` in `materials`; an Arc seen before (same data pointer) is not pushed again.
    pub fn material(&mut self, m: &std::sync::Arc<dyn super::materials::Material + Send + Sync>) -> i32 {
        let key = std::sync::Arc::as_ptr(m) as *const () as usize;
        if let Some(&i) = self.material_ids.get(&key) { return i; }
        let i = self.materials.len() as i32;
        self.materials.push(m.flatten());
        self.material_ids.insert(key, i);
        i
    }
    /// Index of a texture given as tightly packed RGB8 rows, top row first (texture.rs:30 `get_pixel(x, y).to_rgb()`).
    pub fn texture_rgb8(&mut self, width: u32, height: u32, rgb: Vec<u8>) -> i32 {
        assert_eq!(rgb.len(), width as usize * height as usize * 3);
        let i = self.textures.len() as i32;
        self.tex_bytes.push(rgb);
        let p = self.tex_bytes.last().unwrap().as_ptr();
        self.textures.push(mi_texture { width: width as i32, height: height as i32, rgb: p });
        i
    }
    pub fn mesh_index(&self, key: usize) -> Option<i32> { self.mesh_ids.get(&key).copied() }
    pub fn remember_mesh(&mut self, key: usize, index: i32) { self.mesh_ids.insert(key, index); }

    /// The POD view; valid while `self` (and the scene it was flattened from) is alive and unchanged.
    pub fn desc(&self) -> mi_scene_desc {
        mi_scene_desc {
            objects: self.objects.as_ptr(), n_objects: self.objects.len() as i32,
            spheres: self.spheres.as_ptr(), n_spheres: self.spheres.len() as i32,
            triangles: self.triangles.as_ptr(), n_triangles: self.triangles.len() as i32,
            planes: self.planes.as_ptr(), n_planes: self.planes.len() as i32,
            volumes: self.volumes.as_ptr(), n_volumes: self.volumes.len() as i32,
            meshes: self.meshes.as_ptr(), n_meshes: self.meshes.len() as i32,
            materials: self.materials.as_ptr(), n_materials: self.materials.len() as i32,
            textures: self.textures.as_ptr(), n_textures: self.textures.len() as i32,
            boundary_objects: self.boundary_objects.as_ptr(), n_boundary_objects: self.boundary_objects.len() as i32,
            point_light_pos: [0.0, 1.0, 5.0], ambient: [0.1, 0.1, 0.1],   // the caller overwrites both from Scene (tracing.rs:216-217)
        }
    }
}

/// `mi_last_error()` of this thread as a String.
pub fn last_error() -> String {
    unsafe {
        let p = mi_last_error();
        if p.is_null() { String::new() } else { std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned() }
    }
}
