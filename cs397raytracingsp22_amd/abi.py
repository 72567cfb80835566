"""ctypes binding of the C ABI declared in include/mi_rt.h (libmi_rt.so).

This is plumbing only: it mirrors the PODs of mi_rt.h one to one and loads the HIP
library.  There is NO CPU fallback anywhere in this package: if the library is
missing, `load()` raises, and every entry point that needs the GPU fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libmi_rt.so")

MI_TILE = 32

# status codes (mi_status)
MI_RT_ABI_VERSION = 5      # include/mi_rt.h
MI_OK, MI_ERR_INVALID, MI_ERR_UNSUPPORTED, MI_ERR_NO_DEVICE, MI_ERR_HIP, MI_ERR_OOM, MI_ERR_NO_SCENE = 0, -1, -2, -3, -4, -5, -6
# material kinds
MI_MAT_LAMBERTIAN, MI_MAT_METAL, MI_MAT_DIELECTRIC, MI_MAT_PARAMETERIZED, MI_MAT_ISOTROPIC = range(5)
# object kinds
MI_OBJ_SPHERE, MI_OBJ_TRIANGLE, MI_OBJ_PLANE, MI_OBJ_VOLUME, MI_OBJ_MESH, MI_OBJ_SCENE = range(6)
MI_PROJ_ORTHOGRAPHIC, MI_PROJ_PERSPECTIVE = 0, 1
MI_SHADE_PHONG, MI_SHADE_PATHTRACE = 0, 1
MI_VARIANT_DEFAULT, MI_VARIANT_SIMPLE, MI_VARIANT_VOTED, MI_VARIANT_VOTED_DIAG = 0, 1, 3, 4      # 2, 5, 6: removed in ABI 3
MI_VARIANT_WAVEFRONT, MI_VARIANT_RECURSIVE = 7, 8
MI_OPT_NO_TILE_MASKS, MI_OPT_REFERENCE_WALK, MI_OPT_TWO_STAGE, MI_OPT_NO_LIST_TREE = 1, 2, 4, 8
MI_OPT_NO_FINAL_CULL = 16
MI_HEMI_WORLD_RADIUS = 1   # mi_hemisphere_occlusion flags: t_max is a world-space radius
MI_LM_JITTER = 1           # mi_lightmap_texels / mi_bake_lightmap flags: one jittered position per row instead of the texel centre
MI_PV_NORMAL_WEIGHT = 1    # mi_probe_volume.flags: weight the eight corners by how far they lie in front of the surface
MI_LP_F16 = 1              # mi_lightmap_pack / _unpack / _*_packed format: `channels` binary16 per texel (0 is f32: refused there)
MI_LP_RGB9E5 = 2           # ... one u32 per texel, three 9-bit mantissas and a shared 5-bit exponent (3 channels only)
MI_BC6H_BLOCK_BYTES = 16   # mi_lightmap_bc6h_*: one block of MI_BC6H_BLOCK_DIM x MI_BC6H_BLOCK_DIM texels
MI_BC6H_BLOCK_DIM = 4
MI_BC6H_MODE = 3           # the low five bits of the one block mode written and read (two 10-bit direct endpoints, 4-bit indices)
MI_BC6H_MAX_ROUNDS = 4     # mi_lightmap_bc6h_encode: the most least-squares rounds
MI_LS_NEAREST = 1          # mi_lightmap_sample / mi_lightmap_sh_sample flags: the reference's nearest-texel addressing, no interpolation

f3 = C.c_float * 3
f16 = C.c_float * 16
i5 = C.c_int32 * 5


class mi_material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("albedo", f3), ("emission", f3), ("roughness", C.c_float),
                ("metallic", C.c_float), ("idx_of_refraction", C.c_float)]


class mi_object(C.Structure):
    _fields_ = [("kind", C.c_int32), ("index", C.c_int32)]


class mi_sphere(C.Structure):
    _fields_ = [("center", f3), ("radius", C.c_float), ("material", C.c_int32)]


class mi_triangle(C.Structure):
    _fields_ = [("a", f3), ("b", f3), ("c", f3), ("material", C.c_int32)]


class mi_plane(C.Structure):
    _fields_ = [("point", f3), ("normal", f3), ("material", C.c_int32)]


class mi_volume(C.Structure):
    _fields_ = [("boundary_center", f3), ("boundary_radius", C.c_float), ("density", C.c_float),
                ("phase_material", C.c_int32), ("boundary_kind", C.c_int32), ("boundary_index", C.c_int32),
                ("boundary_count", C.c_int32)]


class mi_texture(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("rgb", C.POINTER(C.c_uint8))]


class mi_mesh(C.Structure):
    _fields_ = [("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("texcoords", C.POINTER(C.c_float)), ("indices", C.POINTER(C.c_uint32)),
                ("n_vertices", C.c_int32), ("n_triangles", C.c_int32),
                ("transform", f16), ("inv_transform", f16),
                ("material", C.c_int32), ("textures", i5)]


class mi_scene_desc(C.Structure):
    _fields_ = [("objects", C.POINTER(mi_object)), ("n_objects", C.c_int32),
                ("spheres", C.POINTER(mi_sphere)), ("n_spheres", C.c_int32),
                ("triangles", C.POINTER(mi_triangle)), ("n_triangles", C.c_int32),
                ("planes", C.POINTER(mi_plane)), ("n_planes", C.c_int32),
                ("volumes", C.POINTER(mi_volume)), ("n_volumes", C.c_int32),
                ("meshes", C.POINTER(mi_mesh)), ("n_meshes", C.c_int32),
                ("materials", C.POINTER(mi_material)), ("n_materials", C.c_int32),
                ("textures", C.POINTER(mi_texture)), ("n_textures", C.c_int32),
                ("boundary_objects", C.POINTER(mi_object)), ("n_boundary_objects", C.c_int32),
                ("point_light_pos", f3), ("ambient", f3)]


class mi_camera_desc(C.Structure):
    _fields_ = [("eyepoint", f3), ("view_dir", f3), ("up", f3),
                ("projection_mode", C.c_int32), ("shading_mode", C.c_int32),
                ("path_depth", C.c_uint32), ("path_samples", C.c_uint32),
                ("screen_width", C.c_uint32), ("screen_height", C.c_uint32),
                ("focal_length", C.c_float), ("focus_dist", C.c_float), ("lens_radius", C.c_float),
                ("aa_sample_count", C.c_uint32), ("max_trace_dist", C.c_float), ("gamma", C.c_float)]


class mi_render_opts(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("rank", C.c_int32), ("world", C.c_int32),
                ("variant", C.c_int32), ("want_signature", C.c_int32), ("flags", C.c_uint32),
                ("max_state_bytes", C.c_uint64)]


class mi_probe_volume(C.Structure):
    _fields_ = [("lo", f3), ("hi", f3), ("counts", C.c_uint32 * 3), ("flags", C.c_uint32),
                ("sh", C.c_void_p), ("valid", C.c_void_p)]          # host or device addresses, by the entry point


class mi_lightmap_adaptive(C.Structure):
    _fields_ = [("first_samples", C.c_uint32), ("round_samples", C.c_uint32), ("max_rounds", C.c_uint32),
                ("target_rel", C.c_float), ("target_abs", C.c_float)]


class mi_stats(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("pixels", C.c_uint64), ("tiles", C.c_uint32),
                ("tiles_padded", C.c_uint32), ("kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("scene_bytes", C.c_uint32), ("scene_in_lds", C.c_uint32)]


# every symbol include/mi_rt.h declares (tests check the library exports exactly these)
EXPORTS = [
    "mi_ctx_create", "mi_ctx_destroy", "mi_scene_upload", "mi_render", "mi_compact_size",
    "mi_render_tiles_device", "mi_unpermute_device", "mi_tonemap_device", "mi_last_kernel_ms",
    "mi_reserve", "mi_render_samples_device", "mi_last_pipeline_ms", "mi_last_pipeline_counts", "mi_last_diag", "mi_selftest", "mi_last_error", "mi_abi_version",
    "mi_intersect_rays", "mi_intersect_rays_device", "mi_shade_rays", "mi_shade_rays_device",
    "mi_occluded_rays", "mi_occluded_rays_device",
    "mi_hemisphere_occlusion", "mi_hemisphere_occlusion_device",
    "mi_render_rays", "mi_render_rays_device",
    "mi_render_points", "mi_render_points_device",
    "mi_render_probes", "mi_render_probes_device",
    "mi_lightmap_texels", "mi_lightmap_texels_device", "mi_bake_lightmap",
    "mi_lightmap_finish", "mi_lightmap_finish_device",
    "mi_render_points_moments", "mi_render_points_moments_device", "mi_bake_lightmap_moments",
    "mi_lightmap_finish_var", "mi_lightmap_finish_var_device",
    "mi_lightmap_select", "mi_lightmap_select_device", "mi_lightmap_gather", "mi_lightmap_gather_device",
    "mi_lightmap_merge", "mi_lightmap_merge_device", "mi_lightmap_finish_var_counts", "mi_lightmap_finish_var_counts_device",
    "mi_bake_lightmap_adaptive",
    "mi_probe_volume_sample", "mi_probe_volume_sample_device",
    "mi_render_points_sh", "mi_render_points_sh_device", "mi_bake_lightmap_sh",
    "mi_lightmap_finish_sh", "mi_lightmap_finish_sh_device", "mi_lightmap_sh_eval", "mi_lightmap_sh_eval_device",
    "mi_lightmap_sample", "mi_lightmap_sample_device", "mi_lightmap_sh_sample", "mi_lightmap_sh_sample_device",
    "mi_lightmap_mips", "mi_lightmap_mips_device", "mi_lightmap_sample_lod", "mi_lightmap_sample_lod_device",
    "mi_lightmap_sh_sample_lod", "mi_lightmap_sh_sample_lod_device",
    "mi_lightmap_pack", "mi_lightmap_pack_device", "mi_lightmap_unpack", "mi_lightmap_unpack_device",
    "mi_lightmap_sample_packed", "mi_lightmap_sample_packed_device", "mi_lightmap_sh_sample_packed", "mi_lightmap_sh_sample_packed_device",
    "mi_lightmap_bc6h_encode", "mi_lightmap_bc6h_encode_device", "mi_lightmap_bc6h_decode", "mi_lightmap_bc6h_decode_device",
    "mi_lightmap_sample_bc6h", "mi_lightmap_sample_bc6h_device",
    "mi_multi_create", "mi_multi_create_loopback", "mi_multi_destroy", "mi_multi_device_count", "mi_multi_context", "mi_multi_scene_upload", "mi_multi_reserve", "mi_multi_render",
]

_lib = None


class MiError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"mi_rt error {code}: {msg}")
        self.code = code


def load() -> C.CDLL:
    """Load libmi_rt.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP library has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). "
            "There is no CPU fallback for the render path.")
    # If the process also uses torch (device tensors, torch.distributed), torch's bundled HIP
    # runtime must be the one in the process: load it before libmi_rt.so resolves libamdhip64.
    import sys
    if "torch" in sys.modules or os.environ.get("MI_RT_PRELOAD_TORCH") == "1":
        import torch  # noqa: F401
        if torch.cuda.is_available():
            torch.cuda.init()
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    lib.mi_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.mi_ctx_create.restype = C.c_int
    lib.mi_ctx_destroy.argtypes = [vp]
    lib.mi_ctx_destroy.restype = None
    lib.mi_scene_upload.argtypes = [vp, C.POINTER(mi_scene_desc)]
    lib.mi_scene_upload.restype = C.c_int
    lib.mi_render.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts),
                              vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render.restype = C.c_int
    lib.mi_compact_size.argtypes = [C.POINTER(mi_camera_desc), C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    lib.mi_compact_size.restype = C.c_int
    lib.mi_render_tiles_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts),
                                           vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_tiles_device.restype = C.c_int
    lib.mi_render_samples_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), C.c_uint32, C.c_uint32,
                                             vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_samples_device.restype = C.c_int
    lib.mi_unpermute_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.c_int32, vp, vp, vp]
    lib.mi_unpermute_device.restype = C.c_int
    lib.mi_tonemap_device.argtypes = [vp, C.POINTER(mi_camera_desc), vp, vp, vp]
    lib.mi_tonemap_device.restype = C.c_int
    lib.mi_last_kernel_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.mi_last_kernel_ms.restype = C.c_int
    lib.mi_reserve.argtypes = [vp, C.POINTER(mi_camera_desc), C.c_int32, C.c_uint64]
    lib.mi_reserve.restype = C.c_int
    lib.mi_last_pipeline_ms.argtypes = [vp, C.POINTER(C.c_float)]
    lib.mi_last_pipeline_ms.restype = C.c_int
    lib.mi_last_pipeline_counts.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.mi_last_pipeline_counts.restype = C.c_int
    lib.mi_last_diag.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.mi_last_diag.restype = C.c_int
    lib.mi_selftest.argtypes = [vp, C.POINTER(C.c_uint64)]
    lib.mi_selftest.restype = C.c_int
    # ray queries (added within ABI 5): origins, dirs, t_min, t_max, seed, first_key, then the seven output arrays
    lib.mi_intersect_rays.argtypes = [vp, C.c_uint32, vp, vp, C.c_float, C.c_float, C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, vp, vp]
    lib.mi_intersect_rays.restype = C.c_int
    lib.mi_intersect_rays_device.argtypes = lib.mi_intersect_rays.argtypes + [vp]
    lib.mi_intersect_rays_device.restype = C.c_int
    lib.mi_shade_rays.argtypes = [vp, C.POINTER(mi_camera_desc), C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, vp]
    lib.mi_shade_rays.restype = C.c_int
    lib.mi_shade_rays_device.argtypes = lib.mi_shade_rays.argtypes + [vp]
    lib.mi_shade_rays_device.restype = C.c_int
    lib.mi_occluded_rays.argtypes = [vp, C.c_uint32, vp, vp, C.c_float, C.c_float, vp, C.c_uint32, C.c_uint32, vp]
    lib.mi_occluded_rays.restype = C.c_int
    lib.mi_occluded_rays_device.argtypes = lib.mi_occluded_rays.argtypes + [vp]
    lib.mi_occluded_rays_device.restype = C.c_int
    # hemisphere occlusion (added within ABI 5): n_points, points, normals, first_sample, n_samples, t_min, t_max, flags, seed, first_key,
    # out_open, out_bent
    lib.mi_hemisphere_occlusion.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32,
                                            C.c_uint32, vp, vp]
    lib.mi_hemisphere_occlusion.restype = C.c_int
    lib.mi_hemisphere_occlusion_device.argtypes = lib.mi_hemisphere_occlusion.argtypes + [vp]
    lib.mi_hemisphere_occlusion_device.restype = C.c_int
    # ray-table rendering (added within ABI 5): cam, opts, origins, dirs, rays_per_pixel, then mi_render's outputs / the device form's
    # sample range, accumulator, compact buffer, signatures and stream
    lib.mi_render_rays.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                   vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_rays.restype = C.c_int
    lib.mi_render_rays_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                          C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_rays_device.restype = C.c_int
    # point-table rendering (added within ABI 5): mi_render_rays' argument lists with points / normals / rows_per_pixel for the table
    lib.mi_render_points.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                     vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_points.restype = C.c_int
    lib.mi_render_points_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                            C.c_uint32, C.c_uint32, vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_points_device.restype = C.c_int
    # light probes (added within ABI 5): mi_render_points' argument lists without the normals, with out_sh / d_compact_sh
    lib.mi_render_probes.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, C.c_uint32,
                                     vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_probes.restype = C.c_int
    lib.mi_render_probes_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, C.c_uint32,
                                            C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_probes_device.restype = C.c_int
    # lightmap atlas (added within ABI 5): mesh, width, height, rows, flags, seed, offset, out_points, out_normals, out_triangle (, stream);
    # the bake: cam, opts, mesh, flags, offset, then mi_render's outputs with out_triangle before the stats
    lib.mi_lightmap_texels.argtypes = [vp, C.POINTER(mi_mesh), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                       vp, vp, vp]
    lib.mi_lightmap_texels.restype = C.c_int
    lib.mi_lightmap_texels_device.argtypes = lib.mi_lightmap_texels.argtypes + [vp]
    lib.mi_lightmap_texels_device.restype = C.c_int
    lib.mi_bake_lightmap.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), C.POINTER(mi_mesh), C.c_uint32, C.c_float,
                                     vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_bake_lightmap.restype = C.c_int
    # lightmap finishing (added within ABI 5): width, height, image, points, normals, levels, normal_power_log2, sigma_plane, reach,
    # sigma_color, dilate, out_image, out_valid (, stream)
    lib.mi_lightmap_finish.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, vp, C.c_uint32, C.c_uint32, C.c_float, C.c_float, C.c_float,
                                       C.c_uint32, vp, vp]
    lib.mi_lightmap_finish.restype = C.c_int
    lib.mi_lightmap_finish_device.argtypes = lib.mi_lightmap_finish.argtypes + [vp]
    lib.mi_lightmap_finish_device.restype = C.c_int
    # lightmap variance (added within ABI 5): mi_render_points' / mi_bake_lightmap's argument lists with out_m2 before the plain outputs,
    # mi_render_points_device's with d_compact_m2 behind the accumulator; mi_lightmap_finish's with m2 and samples behind the image,
    # color_floor behind sigma_color and out_var behind out_image
    lib.mi_render_points_moments.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                             vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_points_moments.restype = C.c_int
    lib.mi_render_points_moments_device.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, C.c_uint32,
                                                    C.c_uint32, C.c_uint32, vp, vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_render_points_moments_device.restype = C.c_int
    lib.mi_bake_lightmap_moments.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), C.POINTER(mi_mesh), C.c_uint32,
                                             C.c_float, vp, vp, vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_bake_lightmap_moments.restype = C.c_int
    lib.mi_lightmap_finish_var.argtypes = [vp, C.c_uint32, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_uint32, C.c_uint32, C.c_float,
                                           C.c_float, C.c_float, C.c_float, C.c_uint32, vp, vp, vp]
    lib.mi_lightmap_finish_var.restype = C.c_int
    lib.mi_lightmap_finish_var_device.argtypes = lib.mi_lightmap_finish_var.argtypes + [vp]
    lib.mi_lightmap_finish_var_device.restype = C.c_int
    # adaptive lightmap bake (added within ABI 5): select (the planes, the two targets, capacity, the list, its length, the error plane),
    # gather (the list, the source tables, cw, the compact tables), merge (the list, the round's tables and count, the planes in place),
    # mi_lightmap_finish_var with a counts plane in the place of samples, and mi_bake_lightmap_moments with the adaptive POD and out_counts
    u32, f = C.c_uint32, C.c_float
    lib.mi_lightmap_select.argtypes = [vp, u32, u32, vp, vp, vp, vp, f, f, u32, vp, vp, vp]
    lib.mi_lightmap_select_device.argtypes = lib.mi_lightmap_select.argtypes + [vp]
    lib.mi_lightmap_gather.argtypes = [vp, u32, u32, u32, u32, vp, vp, vp, u32, vp, vp]
    lib.mi_lightmap_gather_device.argtypes = lib.mi_lightmap_gather.argtypes + [vp]
    lib.mi_lightmap_merge.argtypes = [vp, u32, u32, u32, vp, vp, vp, u32, vp, vp, vp]
    lib.mi_lightmap_merge_device.argtypes = lib.mi_lightmap_merge.argtypes + [vp]
    lib.mi_lightmap_finish_var_counts.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, u32, u32, f, f, f, f, u32, vp, vp, vp]
    lib.mi_lightmap_finish_var_counts_device.argtypes = lib.mi_lightmap_finish_var_counts.argtypes + [vp]
    lib.mi_bake_lightmap_adaptive.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), C.POINTER(mi_mesh), u32, f,
                                              C.POINTER(mi_lightmap_adaptive), vp, vp, vp, vp, vp, vp, C.POINTER(mi_stats)]
    for name in ("select", "select_device", "gather", "gather_device", "merge", "merge_device", "finish_var_counts",
                 "finish_var_counts_device"):
        getattr(lib, "mi_lightmap_" + name).restype = C.c_int
    lib.mi_bake_lightmap_adaptive.restype = C.c_int
    # irradiance volumes (added within ABI 5): volume, n_points, points, normals, out_irradiance, out_weight (, stream)
    lib.mi_probe_volume_sample.argtypes = [vp, C.POINTER(mi_probe_volume), C.c_uint32, vp, vp, vp, vp]
    lib.mi_probe_volume_sample.restype = C.c_int
    lib.mi_probe_volume_sample_device.argtypes = lib.mi_probe_volume_sample.argtypes + [vp]
    lib.mi_probe_volume_sample_device.restype = C.c_int
    # directional lightmaps (added within ABI 5): the _moments argument lists with out_sh / d_compact_sh in the place of out_m2 /
    # d_compact_m2; mi_lightmap_finish's with [H][W][9][3] records; n, sh, normals, out_irradiance (, stream)
    lib.mi_render_points_sh.argtypes = lib.mi_render_points_moments.argtypes
    lib.mi_render_points_sh_device.argtypes = lib.mi_render_points_moments_device.argtypes
    lib.mi_bake_lightmap_sh.argtypes = lib.mi_bake_lightmap_moments.argtypes
    lib.mi_lightmap_finish_sh.argtypes = lib.mi_lightmap_finish.argtypes
    lib.mi_lightmap_finish_sh_device.argtypes = lib.mi_lightmap_finish_device.argtypes
    lib.mi_lightmap_sh_eval.argtypes = [vp, u32, vp, vp, vp]
    lib.mi_lightmap_sh_eval_device.argtypes = lib.mi_lightmap_sh_eval.argtypes + [vp]
    for name in ("render_points_sh", "render_points_sh_device", "bake_lightmap_sh", "lightmap_finish_sh", "lightmap_finish_sh_device",
                 "lightmap_sh_eval", "lightmap_sh_eval_device"):
        getattr(lib, "mi_" + name).restype = C.c_int
    # lightmap lookup (added within ABI 5): width, height, channels, image, valid, n, uv, flags, out, out_weight (, stream); the fused SH
    # form: width, height, sh, valid, n, uv, normals, flags, out_irradiance, out_weight (, stream)
    lib.mi_lightmap_sample.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, u32, vp, vp]
    lib.mi_lightmap_sample_device.argtypes = lib.mi_lightmap_sample.argtypes + [vp]
    lib.mi_lightmap_sh_sample.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, u32, vp, vp]
    lib.mi_lightmap_sh_sample_device.argtypes = lib.mi_lightmap_sh_sample.argtypes + [vp]
    for name in ("lightmap_sample", "lightmap_sample_device", "lightmap_sh_sample", "lightmap_sh_sample_device"):
        getattr(lib, "mi_" + name).restype = C.c_int
    # lightmap mips (added within ABI 5): width, height, channels, image, valid, levels, out_mips, out_valid, out_coverage (, stream);
    # the trilinear lookups: lightmap_sample's / lightmap_sh_sample's lists with levels, mips, mip_valid behind valid and lod behind
    # uv / normals
    lib.mi_lightmap_mips.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, vp, vp]
    lib.mi_lightmap_mips_device.argtypes = lib.mi_lightmap_mips.argtypes + [vp]
    lib.mi_lightmap_sample_lod.argtypes = [vp, u32, u32, u32, vp, vp, u32, vp, vp, u32, vp, vp, u32, vp, vp]
    lib.mi_lightmap_sample_lod_device.argtypes = lib.mi_lightmap_sample_lod.argtypes + [vp]
    lib.mi_lightmap_sh_sample_lod.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp]
    lib.mi_lightmap_sh_sample_lod_device.argtypes = lib.mi_lightmap_sh_sample_lod.argtypes + [vp]
    for name in ("lightmap_mips", "lightmap_mips_device", "lightmap_sample_lod", "lightmap_sample_lod_device", "lightmap_sh_sample_lod",
                 "lightmap_sh_sample_lod_device"):
        getattr(lib, "mi_" + name).restype = C.c_int
    # packed lightmaps (added within ABI 5): format, channels, n_texels (u64), in, out (, stream); the packed lookups: format in front of
    # the _lod lookups' lists (lod may be NULL: the level-0 lookup)
    lib.mi_lightmap_pack.argtypes = [vp, u32, u32, C.c_uint64, vp, vp]
    lib.mi_lightmap_pack_device.argtypes = lib.mi_lightmap_pack.argtypes + [vp]
    lib.mi_lightmap_unpack.argtypes = [vp, u32, u32, C.c_uint64, vp, vp]
    lib.mi_lightmap_unpack_device.argtypes = lib.mi_lightmap_unpack.argtypes + [vp]
    lib.mi_lightmap_sample_packed.argtypes = [vp, u32] + lib.mi_lightmap_sample_lod.argtypes[1:]
    lib.mi_lightmap_sample_packed_device.argtypes = lib.mi_lightmap_sample_packed.argtypes + [vp]
    lib.mi_lightmap_sh_sample_packed.argtypes = [vp, u32] + lib.mi_lightmap_sh_sample_lod.argtypes[1:]
    lib.mi_lightmap_sh_sample_packed_device.argtypes = lib.mi_lightmap_sh_sample_packed.argtypes + [vp]
    for name in ("lightmap_pack", "lightmap_pack_device", "lightmap_unpack", "lightmap_unpack_device", "lightmap_sample_packed",
                 "lightmap_sample_packed_device", "lightmap_sh_sample_packed", "lightmap_sh_sample_packed_device"):
        getattr(lib, "mi_" + name).restype = C.c_int
    # BC6H lightmaps (added within ABI 5): width, height, image, valid, rounds, out_blocks; width, height, blocks, out_image; the lookup:
    # mi_lightmap_sample_packed's list without format and channels
    lib.mi_lightmap_bc6h_encode.argtypes = [vp, u32, u32, vp, vp, u32, vp]
    lib.mi_lightmap_bc6h_encode_device.argtypes = lib.mi_lightmap_bc6h_encode.argtypes + [vp]
    lib.mi_lightmap_bc6h_decode.argtypes = [vp, u32, u32, vp, vp]
    lib.mi_lightmap_bc6h_decode_device.argtypes = lib.mi_lightmap_bc6h_decode.argtypes + [vp]
    lib.mi_lightmap_sample_bc6h.argtypes = lib.mi_lightmap_sample_packed.argtypes[:1] + lib.mi_lightmap_sample_packed.argtypes[2:4] + lib.mi_lightmap_sample_packed.argtypes[5:]
    lib.mi_lightmap_sample_bc6h_device.argtypes = lib.mi_lightmap_sample_bc6h.argtypes + [vp]
    for name in ("lightmap_bc6h_encode", "lightmap_bc6h_encode_device", "lightmap_bc6h_decode", "lightmap_bc6h_decode_device",
                 "lightmap_sample_bc6h", "lightmap_sample_bc6h_device"):
        getattr(lib, "mi_" + name).restype = C.c_int
    lib.mi_multi_create.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
    lib.mi_multi_create.restype = C.c_int
    lib.mi_multi_create_loopback.argtypes = [C.c_int, C.c_int, C.POINTER(vp)]
    lib.mi_multi_create_loopback.restype = C.c_int
    lib.mi_multi_destroy.argtypes = [vp]
    lib.mi_multi_destroy.restype = None
    lib.mi_multi_device_count.argtypes = [vp]
    lib.mi_multi_device_count.restype = C.c_int
    lib.mi_multi_context.argtypes = [vp, C.c_int]
    lib.mi_multi_context.restype = vp
    lib.mi_multi_scene_upload.argtypes = [vp, C.POINTER(mi_scene_desc)]
    lib.mi_multi_scene_upload.restype = C.c_int
    lib.mi_multi_reserve.argtypes = [vp, C.POINTER(mi_camera_desc), C.c_uint64]
    lib.mi_multi_reserve.restype = C.c_int
    lib.mi_multi_render.argtypes = [vp, C.POINTER(mi_camera_desc), C.POINTER(mi_render_opts), vp, vp, vp, C.POINTER(mi_stats)]
    lib.mi_multi_render.restype = C.c_int
    lib.mi_last_error.argtypes = []
    lib.mi_last_error.restype = C.c_char_p
    lib.mi_abi_version.argtypes = []
    lib.mi_abi_version.restype = C.c_int
    _lib = lib
    return lib


def check(code: int) -> None:
    if code != MI_OK:
        msg = load().mi_last_error()
        raise MiError(code, msg.decode("utf-8", "replace") if msg else "")
