"""cs397raytracingsp22_amd — MI355X-native path-tracing hot path behind the reference's
Scene / Camera / Material / Intersectable surface (mbk6/CS397RayTracingSP22).

Layout:
  csrc/        HIP kernels (gfx950) + the C-ABI host runtime  -> lib/libmi_rt.so
  abi.py       ctypes binding of include/mi_rt.h
  tracing.py, geometry.py, materials.py, texture.py
               host-side mirror of the reference modules of the same names
  scenes.py    the BASELINE.json configurations
  dist.py      one-process-per-GPU tile sharding + the single RCCL gather

The render path exists only as HIP code: importing this package never falls back to a
CPU implementation, and abi.load() raises when lib/libmi_rt.so has not been built.
"""
from . import abi  # noqa: F401
from .materials import Dielectric, Isotropic, Lambertian, Material, Metal, ParameterizedMaterial  # noqa: F401
from .geometry import ConvexVolume, Intersectable, Plane, Sphere, StaticMesh, Triangle  # noqa: F401
from .texture import Texture  # noqa: F401
from .tracing import Camera, CameraProjectionMode, Context, MultiContext, Scene, ShadingMode, compact_size  # noqa: F401
from .tracing import check_ray_table, equirect_dirs, equirect_ray_table  # noqa: F401
from .tracing import check_point_table, lightmap_jitter, lightmap_texels  # noqa: F401
from .tracing import check_finish_tables, lightmap_finish, lightmap_finish_var  # noqa: F401
from .tracing import check_counts_plane, lightmap_gather, lightmap_merge, lightmap_select  # noqa: F401
from .tracing import check_probe_table, probe_grid, sh9_basis, sh9_irradiance  # noqa: F401
from .tracing import ProbeVolume, check_probe_volume, check_volume_points, probe_volume_sample  # noqa: F401
from .tracing import check_finish_sh_tables, check_sh_eval, lightmap_finish_sh, lightmap_sh_eval  # noqa: F401
from .tracing import check_lightmap_lookup, lightmap_sample, lightmap_sh_sample, shade_hits_baked  # noqa: F401
from .tracing import check_lightmap_lod, check_lightmap_mips, lightmap_mip_layout, lightmap_mips  # noqa: F401
from .tracing import lightmap_sample_lod, lightmap_sh_sample_lod  # noqa: F401
from .tracing import Bc6hLightmap, check_lightmap_bc6h, check_lightmap_bc6h_image, lightmap_bc6h_chain, lightmap_bc6h_decode  # noqa: F401
from .tracing import lightmap_bc6h_encode, lightmap_bc6h_layout, lightmap_bc6h_modes, lightmap_sample_bc6h  # noqa: F401
from .tracing import check_lightmap_packed, lightmap_pack, lightmap_unpack, lightmap_sample_packed, lightmap_sh_sample_packed  # noqa: F401

__all__ = [
    "abi", "Camera", "CameraProjectionMode", "ShadingMode", "Scene", "Context", "MultiContext", "compact_size",
    "Intersectable", "Sphere", "Triangle", "Plane", "ConvexVolume", "StaticMesh",
    "Material", "Lambertian", "Metal", "Dielectric", "ParameterizedMaterial", "Isotropic", "Texture",
    "lightmap_bc6h_layout", "lightmap_bc6h_encode", "lightmap_bc6h_decode", "lightmap_bc6h_modes", "lightmap_bc6h_chain",
    "lightmap_sample_bc6h", "check_lightmap_bc6h", "check_lightmap_bc6h_image", "Bc6hLightmap",
    "lightmap_pack", "lightmap_unpack", "lightmap_sample_packed", "lightmap_sh_sample_packed", "check_lightmap_packed",
    "lightmap_mip_layout", "lightmap_mips", "lightmap_sample_lod", "lightmap_sh_sample_lod", "check_lightmap_mips", "check_lightmap_lod",
]
