"""Host-side mirror of src/util/tracing.rs: `Camera` and `Scene` with the reference's
field names; `Scene.render_to_image()` keeps its meaning (tracing.rs:221-263) and
becomes flatten -> one call through the C ABI (include/mi_rt.h) -> image bytes.

Everything below `render_to_image` — generate_rays, shade_ray, the hit loop, every
intersect_ray / scatter / texture sample — runs in the HIP kernels of csrc/.  There is
no CPU implementation of the path in this package.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional
import numpy as np

from . import abi
from .geometry import FlatBuilder, FlatScene, Intersectable


class CameraProjectionMode:          # tracing.rs:27-30
    Orthographic = abi.MI_PROJ_ORTHOGRAPHIC
    Perspective = abi.MI_PROJ_PERSPECTIVE


class ShadingMode:                   # tracing.rs:32-35
    Phong = abi.MI_SHADE_PHONG
    PathTrace = abi.MI_SHADE_PATHTRACE


@dataclass
class Camera:                        # tracing.rs:138-155, same fields
    eyepoint: tuple = (0.0, 2.0, 5.5)
    view_dir: tuple = (0.0, 0.0, -1.0)
    up: tuple = (0.0, 1.0, 0.0)
    projection_mode: int = CameraProjectionMode.Perspective
    shading_mode: int = ShadingMode.PathTrace
    path_depth: int = 10
    path_samples: int = 1
    screen_width: int = 100
    screen_height: int = 100
    focal_length: float = 0.6
    focus_dist: float = 5.0
    lens_radius: float = 0.0
    aa_sample_count: int = 100
    max_trace_dist: float = 100.0
    gamma: float = 2.0

    def to_pod(self) -> abi.mi_camera_desc:
        c = abi.mi_camera_desc()
        c.eyepoint = abi.f3(*np.asarray(self.eyepoint, np.float32))
        c.view_dir = abi.f3(*np.asarray(self.view_dir, np.float32))
        c.up = abi.f3(*np.asarray(self.up, np.float32))
        c.projection_mode, c.shading_mode = self.projection_mode, self.shading_mode
        c.path_depth, c.path_samples = self.path_depth, self.path_samples
        c.screen_width, c.screen_height = self.screen_width, self.screen_height
        c.focal_length, c.focus_dist, c.lens_radius = self.focal_length, self.focus_dist, self.lens_radius
        c.aa_sample_count = self.aa_sample_count
        c.max_trace_dist, c.gamma = self.max_trace_dist, self.gamma
        return c


@dataclass
class RayHits:
    """Result of Context.intersect_rays: one entry per ray, numpy arrays.  `object` is the index into Scene.objects (-1 = no hit;
    every other array then holds zeros).  With resolve=False only `object` and `distance` are filled, the rest is None."""
    object: np.ndarray                       # [n] int32
    distance: np.ndarray                     # [n] f32, RayHit.distance (object-space t for a StaticMesh)
    hitpoint: Optional[np.ndarray] = None    # [n, 3] f32
    normal: Optional[np.ndarray] = None      # [n, 3] f32, facing the ray (zero inside a ConvexVolume)
    frontface: Optional[np.ndarray] = None   # [n] bool
    has_uv: Optional[np.ndarray] = None      # [n] bool
    uv: Optional[np.ndarray] = None          # [n, 2] f32
    material: Optional[np.ndarray] = None    # [n] structured: kind, albedo, emission, roughness, metallic, idx_of_refraction

    def __len__(self):
        return len(self.object)


# numpy view of abi.mi_material (40 bytes)
MATERIAL_DTYPE = np.dtype([("kind", np.int32), ("albedo", np.float32, 3), ("emission", np.float32, 3), ("roughness", np.float32),
                           ("metallic", np.float32), ("idx_of_refraction", np.float32)])


def check_rays(origins, dirs, t_min: float = 0.001, t_max: float = float("inf")):
    """Input checking of the ray queries (no GPU needed): `origins` and `dirs` as C-contiguous float32 arrays of shape (n, 3) and
    equal length, t_min / t_max as floats that are not NaN.  Directions are NOT normalised (the reference does not either)."""
    o = np.ascontiguousarray(np.asarray(origins, dtype=np.float32))
    d = np.ascontiguousarray(np.asarray(dirs, dtype=np.float32))
    for name, a in (("origins", o), ("dirs", d)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must have shape (n, 3), got {a.shape}")
    if len(o) != len(d):
        raise ValueError(f"origins and dirs differ in length: {len(o)} and {len(d)}")
    if len(o) >= 1 << 32:
        raise ValueError("at most 2^32 - 1 rays per call")
    t_min, t_max = float(t_min), float(t_max)
    if t_min != t_min or t_max != t_max:
        raise ValueError("t_min / t_max must not be NaN")
    return o, d, t_min, t_max


def check_ray_t_max(ray_t_max, n_rays: int):
    """Input checking of mi_occluded_rays' per-ray interval ends (no GPU needed): None stays None; otherwise a C-contiguous float32
    array of shape (n_rays,) without NaN (+inf is legal).  Anything that is not already a real floating-point array or sequence of
    numbers is refused rather than converted."""
    if ray_t_max is None:
        return None
    a = np.asarray(ray_t_max)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"ray_t_max must hold real numbers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"ray_t_max must have shape (n,), got {a.shape}")
    if len(a) != n_rays:
        raise ValueError(f"ray_t_max holds {len(a)} values for {n_rays} rays")
    with np.errstate(over="ignore"):                     # a float64 beyond f32's range becomes +-inf, which is legal
        a = np.ascontiguousarray(a, dtype=np.float32)
    if np.isnan(a).any():
        raise ValueError("ray_t_max must not hold NaN")
    return a


def check_hemisphere(points, normals, n_samples: int, t_min: float = 0.001, t_max: float = float("inf"), flags: int = 0,
                     first_sample: int = 0):
    """Input checking of mi_hemisphere_occlusion (no GPU needed): `points` and `normals` as C-contiguous float32 arrays of shape (n, 3)
    and equal length, n_samples in 1 .. 65535, first_sample + n_samples <= 2^31, t_min / t_max not NaN, flags 0 or
    MI_HEMI_WORLD_RADIUS.  Normals are NOT normalised.  -> (points, normals, n_samples, t_min, t_max, flags, first_sample)."""
    p = np.ascontiguousarray(np.asarray(points, dtype=np.float32))
    n = np.ascontiguousarray(np.asarray(normals, dtype=np.float32))
    for name, a in (("points", p), ("normals", n)):
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must have shape (n, 3), got {a.shape}")
    if len(p) != len(n):
        raise ValueError(f"points and normals differ in length: {len(p)} and {len(n)}")
    if len(p) >= 1 << 32:
        raise ValueError("at most 2^32 - 1 points per call")
    n_samples, first_sample, flags = int(n_samples), int(first_sample), int(flags)
    if not 1 <= n_samples <= 65535:
        raise ValueError(f"n_samples must be in 1 .. 65535, got {n_samples}")
    if first_sample < 0 or first_sample + n_samples > 1 << 31:
        raise ValueError(f"first_sample + n_samples must not exceed 2^31, got {first_sample} + {n_samples}")
    if flags & ~abi.MI_HEMI_WORLD_RADIUS:
        raise ValueError(f"unknown flag bits {flags & ~abi.MI_HEMI_WORLD_RADIUS:#x}")
    t_min, t_max = float(t_min), float(t_max)
    if t_min != t_min or t_max != t_max:
        raise ValueError("t_min / t_max must not be NaN")
    return p, n, n_samples, t_min, t_max, flags, first_sample


def check_shade_camera(cam: "Camera"):
    """Input checking of mi_shade_rays' camera (no GPU needed), the refusals of the library's check_shade_args that concern values:
    path_samples >= 1 (tracing.rs:318 divides by it) and a max_trace_dist that is not NaN (+inf is legal)."""
    if int(cam.path_samples) < 1:
        raise ValueError("path_samples must be >= 1 (tracing.rs:318 divides by it)")
    if float(cam.max_trace_dist) != float(cam.max_trace_dist):
        raise ValueError("max_trace_dist must not be NaN")
    return cam


def check_ray_table(cam: "Camera", origins, dirs):
    """Input checking of ray-table rendering (mi_render_rays), no GPU needed.  `origins` and `dirs` are float32 arrays of shape
    [S, H, W, 3] or [H, W, 3] (= one row) with H, W = cam.screen_height, cam.screen_width and S = 1 (every sample of a pixel uses the
    same ray) or cam.aa_sample_count (sample s uses row s).  Other dtypes are refused, not converted: a table is large.  The camera is
    checked for what the call reads — image size, aa_sample_count in 1..65535 (any value, not only squares), path_depth, path_samples
    (1: the wavefront pipeline), shading_mode (PathTrace), max_trace_dist (not NaN), gamma (finite, > 0); eyepoint .. lens_radius are
    ignored and may hold anything.  Returns (origins, dirs, rays_per_pixel) as C-contiguous [S, H, W, 3] arrays; raises ValueError."""
    return _check_table(cam, origins, dirs, "ray", "origins", "dirs", "rays")


def _check_table(cam: "Camera", first, second, kind: str, first_name: str, second_name: str, unit: str):
    """check_ray_table / check_point_table: the camera fields a table render reads and the two tables' dtype and shape"""
    W, H, aa = int(cam.screen_width), int(cam.screen_height), int(cam.aa_sample_count)
    if not (1 <= W <= 32768 and 1 <= H <= 32768):
        raise ValueError(f"bad image size {W}x{H}")
    if not 1 <= aa <= 0xffff:
        raise ValueError(f"aa_sample_count must be in 1..65535, got {aa}")
    if not 0 <= int(cam.path_depth) <= 0xffff:
        raise ValueError("path_depth must be in 0..65535")
    if int(cam.path_samples) < 1:
        raise ValueError("path_samples must be >= 1 (tracing.rs:318 divides by it)")
    if int(cam.path_samples) != 1:
        raise ValueError(f"{kind}-table rendering runs the wavefront pipeline, path_samples == 1 only: use shade_rays (mi_shade_rays)")
    if cam.shading_mode == ShadingMode.Phong:
        raise ValueError(f"{kind}-table rendering: ShadingMode.Phong is not available for caller-supplied rays (shade_rays has none either)")
    if cam.shading_mode != ShadingMode.PathTrace:
        raise ValueError(f"unknown shading_mode {cam.shading_mode}")
    if float(cam.max_trace_dist) != float(cam.max_trace_dist):
        raise ValueError("max_trace_dist must not be NaN")
    g = float(cam.gamma)
    if not (g > 0.0) or g == float("inf"):
        raise ValueError("gamma must be finite and > 0 (tracing.rs:254 raises to 1/gamma)")
    out = []
    for name, a in ((first_name, first), (second_name, second)):
        a = np.asarray(a)
        if a.dtype != np.float32:
            raise ValueError(f"{name} must be float32, got {a.dtype}")
        if a.ndim == 3:
            a = a[None]
        if a.ndim != 4 or a.shape[1:] != (H, W, 3):
            raise ValueError(f"{name} must have shape [S, {H}, {W}, 3] or [{H}, {W}, 3], got {tuple(np.shape(a))}")
        if a.shape[0] not in (1, aa):
            raise ValueError(f"{name} holds {a.shape[0]} {unit} per pixel: a {kind} table holds 1 row or aa_sample_count = {aa} rows")
        out.append(np.ascontiguousarray(a))
    if out[0].shape != out[1].shape:
        raise ValueError(f"{first_name} and {second_name} differ in shape: {out[0].shape} and {out[1].shape}")
    return out[0], out[1], int(out[0].shape[0])


def check_point_table(cam: "Camera", points, normals):
    """Input checking of point-table rendering (mi_render_points), no GPU needed: check_ray_table for a table of surface points and one
    of normals — float32 arrays of shape [S, H, W, 3] or [H, W, 3] (= one row), S = 1 or cam.aa_sample_count, and the camera fields a table
    render reads.  The values are not looked at: a zero normal marks an empty texel, and non-finite texels are the caller's business (they
    spoil their own pixel only).  Returns (points, normals, rows_per_pixel) as C-contiguous [S, H, W, 3] arrays; raises ValueError."""
    return _check_table(cam, points, normals, "point", "points", "normals", "rows")


def check_probe_table(cam: "Camera", points):
    """Input checking of light-probe rendering (mi_render_probes), no GPU needed: check_point_table for the one table a probe render
    takes — probe positions, float32 of shape [S, H, W, 3] or [H, W, 3] (= one row), S = 1 or cam.aa_sample_count — and the camera fields
    a table render reads.  The values are not looked at: every position is a probe, (0, 0, 0) included, and a non-finite one spoils its
    own probe only.  Returns (points, rows_per_pixel) with points C-contiguous [S, H, W, 3]; raises ValueError."""
    p, _, rows = _check_table(cam, points, points, "probe", "points", "points", "rows")
    return p, rows


SH9_Y0 = 0.28209479177387814        # the real SH basis of order <= 2 in mi_rt.h's order: Y_0; Y_1..3 = SH9_Y1 * (y, z, x);
SH9_Y1 = 0.4886025119029199         # Y_4, 5, 7 = SH9_Y2 * (xy, yz, xz); Y_6 = SH9_Y20 * (3 z^2 - 1); Y_8 = SH9_Y22 * (x^2 - y^2)
SH9_Y2 = 1.0925484305920792
SH9_Y20 = 0.31539156525252005
SH9_Y22 = 0.5462742152960396
SH9_COSINE = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)      # A_l per coefficient: the clamped-cosine lobe's zonal factors


def sh9_basis(dirs) -> np.ndarray:
    """The nine real spherical harmonics of order <= 2 at directions `dirs` [..., 3] (any length: normalised here, in float64), in the
    order and with the constants of mi_render_probes: [..., 9] float64.  Orthonormal over the sphere."""
    d = np.asarray(dirs, np.float64)
    d = d / np.sqrt((d * d).sum(axis=-1, keepdims=True))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, SH9_Y0), SH9_Y1 * y, SH9_Y1 * z, SH9_Y1 * x, SH9_Y2 * x * y, SH9_Y2 * y * z,
                     SH9_Y20 * (3.0 * z * z - 1.0), SH9_Y2 * x * z, SH9_Y22 * (x * x - y * y)], axis=-1)


def sh9_irradiance(sh, normal) -> np.ndarray:
    """Irradiance E(n) = sum_k A_l(k) c_k Y_k(n) from SH L2 radiance coefficients `sh` [..., 9, C] (render_probes' first result) for a
    normal [3] or one normal per probe [..., 3]: [..., C] float64.  A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4 (Ramamoorthi & Hanrahan 2001):
    constant radiance L gives pi L.  Divide by pi and multiply by the albedo for a Lambertian surface's outgoing radiance."""
    w = sh9_basis(normal) * SH9_COSINE                                  # [..., 9]
    return (np.asarray(sh, np.float64) * w[..., None]).sum(axis=-2)


def probe_grid(lo, hi, counts, width: Optional[int] = None):
    """A regular grid of light probes inside the box [lo, hi] as a probe table: (points [H, W, 3] float32, n).  counts = (nx, ny, nz);
    probe (i, j, k) sits at the centre of its cell, lo + (i + 0.5, j + 0.5, k + 0.5) / counts * (hi - lo), and has the number
    (k * ny + j) * nx + i (x runs fastest).  The n = nx ny nz probes fill the table row-major: W = `width`, or, when width is None, the
    multiple of 32 next above sqrt(n) (the renderer works in 32 x 32 tiles: a squarish table wastes the fewest lanes, a single row 31 of
    every 32); H = ceil(n / W).  The H W - n padding slots repeat the last probe, so every slot is a finite position; only the first n
    results (reshape(-1, ...)[:n]) mean anything."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    nx, ny, nz = (int(c) for c in counts)
    if min(nx, ny, nz) < 1:
        raise ValueError(f"counts must all be >= 1, got {(nx, ny, nz)}")
    n = nx * ny * nz
    W = min(32768, 32 * int(np.ceil(np.sqrt(n) / 32.0))) if width is None else int(width)
    if not 1 <= W <= 32768:
        raise ValueError(f"width must be in 1..32768, got {W}")
    H = (n + W - 1) // W
    if H > 32768:
        raise ValueError(f"{n} probes do not fit {W} columns x 32768 rows")
    ax = [lo[a] + (np.arange(c) + 0.5) / c * (hi[a] - lo[a]) for a, c in enumerate((nx, ny, nz))]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    pts = np.stack([x, y, z], axis=-1).reshape(n, 3)
    pts = np.concatenate([pts, np.repeat(pts[-1:], H * W - n, axis=0)])
    return np.ascontiguousarray(pts.reshape(H, W, 3), np.float32), n


# K_k of mi_probe_volume_sample: the clamped-cosine lobe's A_l times the basis constant of Y_k, rounded from f64 to f32
PV_K = np.array([0.886226925452758] + [1.0233267079464885] * 3 + [0.8580855308097834] * 2 + [0.24770795610037571, 0.8580855308097834,
                0.4290427654048917], np.float64).astype(np.float32)
PV_MAX_COUNT = 1024
PV_MAX_PROBES = 1 << 22


def check_probe_volume(lo, hi, counts, sh, valid=None, flags: int = 0):
    """Input checking of an irradiance volume (mi_probe_volume_sample), no GPU needed: the box [lo, hi] probe_grid was given (finite,
    hi > lo on every axis, as float32), counts = (nx, ny, nz) each in 1 .. 1024 with at most 2^22 probes, sh [n, 9, 3] float32 (the first
    n = nx ny nz records of render_probes' sh), valid None or [n] (0 = the probe takes no part), flags 0 or abi.MI_PV_NORMAL_WEIGHT.
    Returns (lo [3] f32, hi [3] f32, (nx, ny, nz), sh [n, 9, 3] f32 contiguous, valid [n] uint8 or None, flags); raises ValueError."""
    lo32, hi32 = np.asarray(lo, np.float32).reshape(-1), np.asarray(hi, np.float32).reshape(-1)
    if lo32.shape != (3,) or hi32.shape != (3,):
        raise ValueError("lo and hi must have three components each")
    if not (np.isfinite(lo32).all() and np.isfinite(hi32).all()):
        raise ValueError(f"lo and hi must be finite, got {lo32} and {hi32}")
    if not (hi32 > lo32).all():
        raise ValueError(f"hi must be above lo on every axis, got lo {lo32} and hi {hi32}")
    try:
        nx, ny, nz = (int(c) for c in counts)
    except (TypeError, ValueError):
        raise ValueError(f"counts must be three integers, got {counts!r}") from None
    if not all(1 <= c <= PV_MAX_COUNT for c in (nx, ny, nz)):
        raise ValueError(f"counts must all be in 1 .. {PV_MAX_COUNT}, got {(nx, ny, nz)}")
    n = nx * ny * nz
    if n > PV_MAX_PROBES:
        raise ValueError(f"{n} probes exceed 2^22")
    flags = int(flags)
    if flags & ~abi.MI_PV_NORMAL_WEIGHT:
        raise ValueError(f"unknown flag bits {flags & ~abi.MI_PV_NORMAL_WEIGHT:#x}")
    sh32 = np.ascontiguousarray(sh, np.float32)
    if sh32.shape != (n, 9, 3):
        raise ValueError(f"sh must be [{n}, 9, 3] for counts {(nx, ny, nz)}, got {sh32.shape}")
    v8 = None
    if valid is not None:
        v8 = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        if v8.shape != (n,):
            raise ValueError(f"valid must be [{n}], got {v8.shape}")
    return lo32, hi32, (nx, ny, nz), sh32, v8, flags


def check_volume_points(points, normals):
    """(points [n, 3] f32, normals [n, 3] f32, leading shape) of the surface points an irradiance volume is sampled at: two float32 arrays
    of one shape [..., 3] (an atlas table [rows, H, W, 3] is one).  The values are not looked at: an all-zero normal is an empty texel,
    a non-finite point or normal spoils its own result only.  Raises ValueError."""
    P, N = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    if P.ndim < 1 or P.shape[-1] != 3 or N.shape != P.shape:
        raise ValueError(f"points and normals must be [..., 3] arrays of one shape, got {P.shape} and {N.shape}")
    if P.size // 3 >= 1 << 32:
        raise ValueError(f"{P.size // 3} points exceed 2^32 - 1")
    return np.ascontiguousarray(P.reshape(-1, 3)), np.ascontiguousarray(N.reshape(-1, 3)), P.shape[:-1]


def probe_volume_sample(lo, hi, counts, sh, points, normals, valid=None, flags: int = 0):
    """Sample an irradiance volume on the host (numpy only): trilinear interpolation of a probe_grid of SH L2 radiance probes at surface
    points, convolved with the clamped cosine lobe about each point's normal.  This is the DEFINITION of mi_probe_volume_sample, which
    equals it bit for bit.  Arguments as check_probe_volume and check_volume_points.  Returns (E [..., 3] f32, weight [...] f32).
    Everything is f32, one rounding per operation (+ - *, IEEE / and sqrt, floor, fmin, fmax), in the order written below.
    Per axis a: cell = (hi - lo) / n, inv = n / (hi - lo).  Prepared record r[q][k][c] = sh[q][k][c] * PV_K[k].
    An all-zero normal gives E = +0 and weight 0.  Otherwise (x, y, z) = n / sqrt((nx nx + ny ny) + nz nz) and
    b = (1, y, z, x, x y, y z, 3 (z z) - 1, x z, x x - y y).  Cell: g = (p - lo) * inv - 0.5, clamped by fmin(fmax(g, 0), n - 1) (which
    also keeps every index in range for NaN and infinite points), i0 = min(floor(g), max(n - 2, 0)), f = g - i0.  The eight corners, dz
    outer, dy, dx inner: i = min(i0 + d, n - 1), w_a = f or 1 - f, w = (w_x w_y) w_z, w = 0 for an invalid probe; with
    MI_PV_NORMAL_WEIGHT D = (lo + (i + 0.5) cell) - p, dd = (Dx Dx + Dy Dy) + Dz Dz and, when dd > 0,
    t = ((Dx x + Dy y) + Dz z) / sqrt(dd), h = (t + 1) 0.5, w = w (h h + 0.2).  e[c] = b0 r[0][c] + ... + b8 r[8][c] left to right,
    acc += w e, sw += w.  E = acc / sw when sw > 0, else +0; weight = sw."""
    f32 = np.float32
    lo, hi, cnt, sh, valid, flags = check_probe_volume(lo, hi, counts, sh, valid, flags)
    P, N, shape = check_volume_points(points, normals)
    n_pts = len(P)
    with np.errstate(all="ignore"):
        nf = np.array(cnt, np.float32)
        ext = hi - lo
        cell, inv = ext / nf, nf / ext
        rec = sh * PV_K[None, :, None]
        ok = np.ones(len(sh), bool) if valid is None else valid != 0
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        covered = ~((nx == 0) & (ny == 0) & (nz == 0))
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        x, y, z = nx / l, ny / l, nz / l
        d = (x, y, z)
        b = (np.ones(n_pts, f32), y, z, x, x * y, y * z, f32(3.0) * (z * z) - f32(1.0), x * z, x * x - y * y)
        idx, wa, DD, Dn = [], [], [], []
        for a in range(3):
            n = cnt[a]
            g = (P[:, a] - lo[a]) * inv[a] - f32(0.5)
            g = np.fmin(np.fmax(g, f32(0.0)), f32(n - 1))
            i0 = np.minimum(np.floor(g).astype(np.int64), max(n - 2, 0))
            f = g - i0.astype(f32)
            ia = [np.minimum(i0 + dd, n - 1) for dd in (0, 1)]
            D = [(lo[a] + (i.astype(f32) + f32(0.5)) * cell[a]) - P[:, a] for i in ia]
            idx.append(ia); wa.append((f32(1.0) - f, f))
            DD.append([Di * Di for Di in D]); Dn.append([Di * d[a] for Di in D])
        acc = np.zeros((n_pts, 3), f32)
        sw = np.zeros(n_pts, f32)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    q = (idx[2][dz] * cnt[1] + idx[1][dy]) * cnt[0] + idx[0][dx]
                    r = rec[q]                                                     # [n_pts, 9, 3]
                    w = (wa[0][dx] * wa[1][dy]) * wa[2][dz]
                    w = np.where(ok[q], w, f32(0.0))
                    if flags & abi.MI_PV_NORMAL_WEIGHT:
                        dd = (DD[0][dx] + DD[1][dy]) + DD[2][dz]
                        t = ((Dn[0][dx] + Dn[1][dy]) + Dn[2][dz]) / np.sqrt(dd)
                        h = (t + f32(1.0)) * f32(0.5)
                        w = np.where(dd > 0, w * (h * h + f32(0.2)), w)
                    e = b[0][:, None] * r[:, 0, :]
                    for k in range(1, 9):
                        e = e + b[k][:, None] * r[:, k, :]
                    acc = acc + w[:, None] * e
                    sw = sw + w
        E = np.where((sw > 0)[:, None], acc / sw[:, None], f32(0.0))
        E = np.where(covered[:, None], E, f32(0.0))
        sw = np.where(covered, sw, f32(0.0))
    assert E.dtype == np.float32 and sw.dtype == np.float32
    return np.ascontiguousarray(E.reshape(shape + (3,))), np.ascontiguousarray(sw.reshape(shape))


@dataclass
class ProbeVolume:
    """An irradiance volume: a probe_grid of SH L2 radiance probes ready to be sampled.  lo / hi / counts are what probe_grid was given,
    sh [n, 9, 3] f32 the first n records of render_probes' sh, valid None or [n] (0 = the probe takes no part: the caller decides, e.g.
    probes inside geometry).  Scene.irradiance_volume makes one."""
    lo: np.ndarray
    hi: np.ndarray
    counts: tuple
    sh: np.ndarray
    valid: Optional[np.ndarray] = None

    def __post_init__(self):
        self.lo, self.hi, self.counts, self.sh, self.valid, _ = check_probe_volume(self.lo, self.hi, self.counts, self.sh, self.valid)

    def sample(self, points, normals, normal_weight: bool = False, want_weight: bool = False, ctx: Optional["Context"] = None,
               device: int = 0):
        """The irradiance at surface points ([..., 3] f32 each; an atlas table from lightmap_texels goes in as it stands: its empty
        texels come back zero) on the GPU (mi_probe_volume_sample): E [..., 3] f32, or with want_weight (E, weight [...]) — weight 0
        marks a point all of whose corners were invalid.  normal_weight sets MI_PV_NORMAL_WEIGHT: corners in front of the surface count
        more.  `ctx`: a Context to run on (one is made on `device` and closed otherwise).  Divide by pi and multiply by the albedo for
        a Lambertian surface's outgoing radiance."""
        own = ctx is None
        c = Context(device) if own else ctx
        try:
            E, w = c.probe_volume_sample(self, points, normals, flags=abi.MI_PV_NORMAL_WEIGHT if normal_weight else 0)
        finally:
            if own:
                c.close()
        return (E, w) if want_weight else E

    def sample_host(self, points, normals, normal_weight: bool = False):
        """The same on the host (probe_volume_sample, the definition): (E, weight)."""
        return probe_volume_sample(self.lo, self.hi, self.counts, self.sh, points, normals, self.valid,
                                   abi.MI_PV_NORMAL_WEIGHT if normal_weight else 0)


def _lowbias32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _rotl32(x, k: int):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def lightmap_jitter(width: int, height: int, rows: int, seed: int) -> np.ndarray:
    """The sample positions of a jittered lightmap atlas (MI_LM_JITTER), [rows, H, W, 2] float32 in [0, 1): (jx, jy) of row r of texel
    (x, y) are the first two gen_range(0.0..1.0) draws of the fresh stream (seed, 2 W H + y W + x, r) — DESIGN.md "RNG" restated in numpy:
    three rounds of lowbias32 key xoroshiro64**, a draw is bits(0x3f800000 | u32 >> 9) * 1 + (0 - 1).  The sample lies at
    u = (x + jx) / W, v = 1 - (y + jy) / H; lightmap_texels(jitter=...) takes the array."""
    W, H, R = int(width), int(height), int(rows)
    if W < 1 or H < 1 or R < 1:
        raise ValueError("width, height and rows must be >= 1")
    if 3 * W * H > 1 << 31:
        raise ValueError("3 * width * height exceeds 2^31: the jitter streams' keys end at 3 W H")
    with np.errstate(over="ignore"):
        u32 = np.uint32
        k0 = _lowbias32(np.asarray(int(seed) & 0xffffffff, u32) ^ u32(0x68e31da4))
        pixel = (2 * W * H + np.arange(W * H, dtype=np.int64)).astype(u32).reshape(1, H, W)
        sample = np.arange(R, dtype=u32).reshape(R, 1, 1)
        p0 = _lowbias32(pixel + k0)
        p1 = _lowbias32(p0 ^ u32(0xb5297a4d))
        s0 = _lowbias32(p0 + sample * u32(0x9e3779b9))
        s1 = _lowbias32(p1 ^ (sample * u32(0x85ebca6b)))
        s1 = np.where((s0 | s1) == 0, u32(1), s1)
        out = np.empty((R, H, W, 2), np.float32)
        for k in range(2):
            word = _rotl32(s0 * u32(0x9e3779bb), 5) * u32(5)
            s1 = s1 ^ s0
            s0, s1 = _rotl32(s0, 26) ^ s1 ^ (s1 << u32(9)), _rotl32(s1, 13)
            out[..., k] = (u32(0x3f800000) | (word >> u32(9))).view(np.float32) * np.float32(1.0) + np.float32(0.0 - 1.0)
    return out


def lightmap_texels(positions, normals, texcoords, indices, width: int, height: int, transform=None, offset: float = 0.0, jitter=None,
                    with_triangle: bool = False):
    """The point table of a mesh's lightmap, on the host (numpy only): (points [H, W, 3] f32, normals [H, W, 3] f32, covered [H, W] bool)
    for render_points.  `positions`, `normals` [V, 3], `texcoords` [V, 2] and `indices` [T, 3] are a single-index triangle mesh
    (objload.Mesh's arrays, flat or shaped).  Texel (x, y) has its centre at u = (x + 0.5) / W, v = 1 - (y + 0.5) / H: the inverse of
    Texture::sample's x = floor(u W), y = floor((1 - v) H) (texture.rs:28-29), so the baked image, loaded as that mesh's texture, puts
    every texel back where it was gathered.  A texel is covered when its centre lies inside or on the edge of a triangle in uv space
    (edge functions in f64, >= 0); where triangles overlap or share an edge the LOWEST triangle index wins; triangles without area in uv
    cover nothing.  Point and normal are the barycentric interpolation of the triangle's vertices, taken through `transform` (a 4 x 4
    matrix indexed [row, col] as cgmath.py builds them, e.g. StaticMesh.transform; None = identity): points as points, normals through
    the inverse transpose of its upper 3 x 3, then normalised.  The point is moved by `offset` along that unit normal (mi_render_points
    uses the origin as given: a small positive offset keeps the sample rays clear of their own surface).  Uncovered texels — and texels
    whose interpolated normal has no length — have a zero normal and a zero point: the empty-texel mark of mi_render_points.
    `jitter` ([rows, H, W, 2], e.g. lightmap_jitter's) moves the sample of row r of texel (x, y) from the centre to
    u = (x + jx) / W, v = 1 - (y + jy) / H and gives every table a leading [rows] axis: what mi_lightmap_texels makes on the GPU with
    MI_LM_JITTER.  with_triangle adds a fourth result: the winning triangle's index per sample, int32, -1 where not covered."""
    if jitter is not None:
        return _lightmap_texels_jittered(positions, normals, texcoords, indices, width, height, transform, offset, jitter, with_triangle)
    if with_triangle:
        H_, W_ = int(height), int(width)
        out = _lightmap_texels_jittered(positions, normals, texcoords, indices, width, height, transform, offset,
                                        np.full((1, max(H_, 0), max(W_, 0), 2), 0.5, np.float32), True)
        return tuple(t[0] for t in out)
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("width and height must be >= 1")
    P = np.asarray(positions, np.float64).reshape(-1, 3)
    N = np.asarray(normals, np.float64).reshape(-1, 3)
    T = np.asarray(texcoords, np.float64).reshape(-1, 2)
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    if not (len(P) == len(N) == len(T)):
        raise ValueError(f"positions, normals and texcoords must describe the same vertices, got {len(P)}, {len(N)} and {len(T)}")
    if I.size and (I.min() < 0 or I.max() >= len(P)):
        raise ValueError("indices out of range")
    M = np.eye(4) if transform is None else np.asarray(transform, np.float64).reshape(4, 4)
    NM = np.linalg.inv(M[:3, :3]).T
    cu = (np.arange(W) + 0.5) / W                                       # texel centres
    cv = 1.0 - (np.arange(H) + 0.5) / H
    pts = np.zeros((H, W, 3), np.float64)
    nrm = np.zeros((H, W, 3), np.float64)
    covered = np.zeros((H, W), bool)
    for a, b, c in I:
        (ua, va), (ub, vb), (uc, vc) = T[a], T[b], T[c]
        area = (ub - ua) * (vc - va) - (vb - va) * (uc - ua)
        if area == 0.0 or not np.isfinite(area):
            continue
        # the texel columns / rows whose centres can lie in the triangle's uv box (one texel of slack: the edge functions decide)
        x0 = max(0, int(np.floor(min(ua, ub, uc) * W - 0.5)) - 1)
        x1 = min(W - 1, int(np.ceil(max(ua, ub, uc) * W - 0.5)) + 1)
        y0 = max(0, int(np.floor((1.0 - max(va, vb, vc)) * H - 0.5)) - 1)
        y1 = min(H - 1, int(np.ceil((1.0 - min(va, vb, vc)) * H - 0.5)) + 1)
        if x0 > x1 or y0 > y1:
            continue
        u, v = np.meshgrid(cu[x0:x1 + 1], cv[y0:y1 + 1])
        sgn = 1.0 if area > 0.0 else -1.0
        ea = ((ub - u) * (vc - v) - (vb - v) * (uc - u)) * sgn           # weight of vertex a, times |area|
        eb = ((uc - u) * (va - v) - (vc - v) * (ua - u)) * sgn
        ec = ((ua - u) * (vb - v) - (va - v) * (ub - u)) * sgn
        take = (ea >= 0.0) & (eb >= 0.0) & (ec >= 0.0) & ~covered[y0:y1 + 1, x0:x1 + 1]
        if not take.any():
            continue
        tot = ea + eb + ec
        wa, wb, wc = (ea / tot)[take], (eb / tot)[take], (ec / tot)[take]
        yy, xx = np.nonzero(take)
        pts[y0 + yy, x0 + xx] = wa[:, None] * P[a] + wb[:, None] * P[b] + wc[:, None] * P[c]
        nrm[y0 + yy, x0 + xx] = wa[:, None] * N[a] + wb[:, None] * N[b] + wc[:, None] * N[c]
        covered[y0 + yy, x0 + xx] = True
    pts = pts @ M[:3, :3].T + M[:3, 3]
    nrm = nrm @ NM.T
    length = np.sqrt((nrm * nrm).sum(axis=-1))
    covered &= np.isfinite(length) & (length > 0.0)
    nrm = nrm / np.where(covered, length, 1.0)[..., None]
    pts = pts + float(offset) * nrm
    pts[~covered] = 0.0
    nrm[~covered] = 0.0
    return np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(nrm, np.float32), covered


def _lightmap_texels_jittered(positions, normals, texcoords, indices, width, height, transform, offset, jitter, with_triangle):
    """lightmap_texels with one sample position per (row, texel): the same f64 expressions in the same order, the sample's (u, v) in place
    of the centre's, the triangle's texel box widened to every texel a sample of which can lie in its uv box."""
    W, H = int(width), int(height)
    if W < 1 or H < 1:
        raise ValueError("width and height must be >= 1")
    J = np.asarray(jitter, np.float64)
    if J.ndim != 4 or J.shape[1:] != (H, W, 2) or J.shape[0] < 1:
        raise ValueError(f"jitter must be [rows, {H}, {W}, 2], got {list(J.shape)}")
    R = J.shape[0]
    P = np.asarray(positions, np.float64).reshape(-1, 3)
    N = np.asarray(normals, np.float64).reshape(-1, 3)
    T = np.asarray(texcoords, np.float64).reshape(-1, 2)
    I = np.asarray(indices, np.int64).reshape(-1, 3)
    if not (len(P) == len(N) == len(T)):
        raise ValueError(f"positions, normals and texcoords must describe the same vertices, got {len(P)}, {len(N)} and {len(T)}")
    if I.size and (I.min() < 0 or I.max() >= len(P)):
        raise ValueError("indices out of range")
    M = np.eye(4) if transform is None else np.asarray(transform, np.float64).reshape(4, 4)
    NM = np.linalg.inv(M[:3, :3]).T
    U = (np.arange(W)[None, None, :] + J[..., 0]) / W                     # [R, H, W] sample positions
    V = 1.0 - (np.arange(H)[None, :, None] + J[..., 1]) / H
    pts = np.zeros((R, H, W, 3), np.float64)
    nrm = np.zeros((R, H, W, 3), np.float64)
    tri = np.full((R, H, W), -1, np.int32)
    for k, (a, b, c) in enumerate(I):
        (ua, va), (ub, vb), (uc, vc) = T[a], T[b], T[c]
        area = (ub - ua) * (vc - va) - (vb - va) * (uc - ua)
        if area == 0.0 or not np.isfinite(area):
            continue
        fx0, fx1 = np.floor(min(ua, ub, uc) * W) - 1, np.floor(max(ua, ub, uc) * W) + 1
        fy0, fy1 = np.floor((1.0 - max(va, vb, vc)) * H) - 1, np.floor((1.0 - min(va, vb, vc)) * H) + 1
        if not (fx1 >= 0 and fx0 <= W - 1 and fy1 >= 0 and fy0 <= H - 1):
            continue
        x0, x1, y0, y1 = int(max(fx0, 0)), int(min(fx1, W - 1)), int(max(fy0, 0)), int(min(fy1, H - 1))
        u, v = U[:, y0:y1 + 1, x0:x1 + 1], V[:, y0:y1 + 1, x0:x1 + 1]
        sgn = 1.0 if area > 0.0 else -1.0
        ea = ((ub - u) * (vc - v) - (vb - v) * (uc - u)) * sgn
        eb = ((uc - u) * (va - v) - (vc - v) * (ua - u)) * sgn
        ec = ((ua - u) * (vb - v) - (va - v) * (ub - u)) * sgn
        take = (ea >= 0.0) & (eb >= 0.0) & (ec >= 0.0) & (tri[:, y0:y1 + 1, x0:x1 + 1] < 0)
        if not take.any():
            continue
        tot = ea + eb + ec
        wa, wb, wc = (ea / tot)[take], (eb / tot)[take], (ec / tot)[take]
        rr, yy, xx = np.nonzero(take)
        pts[rr, y0 + yy, x0 + xx] = wa[:, None] * P[a] + wb[:, None] * P[b] + wc[:, None] * P[c]
        nrm[rr, y0 + yy, x0 + xx] = wa[:, None] * N[a] + wb[:, None] * N[b] + wc[:, None] * N[c]
        tri[rr, y0 + yy, x0 + xx] = k
    pts = pts @ M[:3, :3].T + M[:3, 3]
    nrm = nrm @ NM.T
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((nrm * nrm).sum(axis=-1))
    covered = (tri >= 0) & np.isfinite(length) & (length > 0.0)
    nrm = nrm / np.where(covered, length, 1.0)[..., None]
    pts = pts + float(offset) * nrm
    pts[~covered] = 0.0
    nrm[~covered] = 0.0
    tri[~covered] = -1
    out = (np.ascontiguousarray(pts, np.float32), np.ascontiguousarray(nrm, np.float32), covered)
    return out + (tri,) if with_triangle else out


_LMF_TAPS = tuple((dy, dx) for dy in range(-2, 3) for dx in range(-2, 3))                          # dy outer, dx inner
_LMF_RING = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0))        # the 8-neighbours, same order
_LMV_BLUR = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1))                              # dy outer, dx inner, the centre included


def _centre_table(table):
    """lightmap_texels' [1, H, W, 3] centre table as [H, W, 3]; any other array as it is"""
    t = np.asarray(table)
    return t[0] if t.ndim == 4 and t.shape[0] == 1 else t


def check_finish_tables(image, points, normals):
    """(image, points, normals) as contiguous float32 [H, W, 3] arrays of one shape, 1 <= W, H <= 32768, for lightmap_finish"""
    img = np.ascontiguousarray(image, np.float32)
    P = np.ascontiguousarray(points, np.float32)
    N = np.ascontiguousarray(normals, np.float32)
    if img.ndim != 3 or img.shape[2] != 3 or P.shape != img.shape or N.shape != img.shape:
        raise ValueError(f"image, points and normals must be [H, W, 3] arrays of one shape, got {img.shape}, {P.shape} and {N.shape}")
    if not (1 <= img.shape[0] <= 32768 and 1 <= img.shape[1] <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {img.shape[1]} x {img.shape[0]}")
    return img, P, N


# The building blocks of lightmap_finish, lightmap_finish_sh, lightmap_finish_var and lightmap_select: each rule of those definitions is
# written once, here.  All f32, one rounding per operation, in the order written; the callers hold np.errstate(all="ignore").
def _lm_covered(N):
    """A texel is covered when its normal is not all-zero (either sign of zero is empty)"""
    return (N[..., 0] != 0) | (N[..., 1] != 0) | (N[..., 2] != 0)


def _lmv_variance(mean, M2, n, covered, few):
    """The variance of the mean: v_c = max(0, m2_c - mean_c mean_c) / (n - 1), V = (v_r + v_g) + v_b, with n one number or the texels' own
    [H, W] counts; `few` where n < 2, +0.0 on empty texels"""
    f32 = np.float32
    n = np.asarray(n).astype(np.int64)
    d = np.maximum(n - 1, 1).astype(f32)
    v3 = np.fmax(f32(0.0), M2 - mean * mean) / d[..., None]
    V = np.where(n >= 2, (v3[..., 0] + v3[..., 1]) + v3[..., 2], few)
    return np.where(covered, V, f32(0.0)).astype(f32)


def _lmv_blur(V, N, covered, b):
    """(bs, bw): the sums g V_q and g over the nine neighbours at spacing b that lie in the image and are covered, dy outer, dx inner,
    g = G3[dy] G3[dx].  Meaningful on covered texels only."""
    f32 = np.float32
    G3 = (f32(0.25), f32(0.5), f32(0.25))
    H, W = V.shape
    vb, nb = np.pad(V, b), np.pad(N, ((b, b), (b, b), (0, 0)))
    bs = np.zeros((H, W), f32)
    bw = np.zeros((H, W), f32)
    for dy, dx in _LMV_BLUR:
        ys, xs = b + b * dy, b + b * dx
        vq, nq = vb[ys:ys + H, xs:xs + W], nb[ys:ys + H, xs:xs + W]
        btake = covered & _lm_covered(nq)
        g = G3[dy + 1] * G3[dx + 1]
        bs = np.where(btake, bs + g * vq, bs)
        bw = np.where(btake, bw + g, bw)
    return bs, bw


def _lmf_level(cur, P, N, covered, s, npow, sig_p, rch, den, V=None):
    """One a-trous level at step s of an image [H, W, C], C >= 3: every channel takes the same weights, whose colour distance is taken from
    the first three and divided by `den`, one number or an [H, W] plane read at p.  With a variance plane V also sv = sv + (w w) V_q.
    Returns (sc / sw, sv / (sw sw) or None), +0.0 on empty texels."""
    f32 = np.float32
    zero, one = f32(0.0), f32(1.0)
    H5 = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))
    H, W, C = cur.shape
    r = rch * f32(s)
    rr = r * r
    pad = 2 * s
    cpad, ppad, npad = (np.pad(t, ((pad, pad), (pad, pad), (0, 0))) for t in (cur, P, N))      # beyond the image: empty texels
    sw = np.zeros((H, W), f32)
    sc = np.zeros((H, W, C), f32)
    if V is not None:
        vpad = np.pad(V, pad)
        sv = np.zeros((H, W), f32)
    for dy, dx in _LMF_TAPS:
        ys, xs = pad + s * dy, pad + s * dx
        cq, pq, nq = (t[ys:ys + H, xs:xs + W] for t in (cpad, ppad, npad))
        take = covered & _lm_covered(nq)
        D = pq - P
        d2 = (D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1]) + D[..., 2] * D[..., 2]
        if dx != 0 or dy != 0:                # the centre always passes (0 <= 0; inf * 0 must not reject it)
            take = take & (d2 <= rr * f32(dx * dx + dy * dy))
        h = H5[dy + 2] * H5[dx + 2]
        wn = np.fmax(zero, (N[..., 0] * nq[..., 0] + N[..., 1] * nq[..., 1]) + N[..., 2] * nq[..., 2])
        for _ in range(npow):
            wn = wn * wn
        dpl = np.abs((N[..., 0] * D[..., 0] + N[..., 1] * D[..., 1]) + N[..., 2] * D[..., 2])
        wp = np.fmax(zero, one - dpl / sig_p)
        dc = (np.abs(cq[..., 0] - cur[..., 0]) + np.abs(cq[..., 1] - cur[..., 1])) + np.abs(cq[..., 2] - cur[..., 2])
        wc = np.fmax(zero, one - dc / den)
        w = ((h * wn) * wp) * wc
        sw = np.where(take, sw + w, sw)
        sc = np.where(take[..., None], sc + w[..., None] * cq, sc)
        if V is not None:
            vq = vpad[ys:ys + H, xs:xs + W]
            sv = np.where(take, sv + (w * w) * vq, sv)
    out = np.where(covered[..., None], sc / sw[..., None], zero)
    return out, None if V is None else np.where(covered, sv / (sw * sw), zero)


def _lmf_dilate(cur, covered, passes):
    """`passes` dilation passes of an image [H, W, C] whose valid texels are the covered ones: (image, valid)"""
    f32 = np.float32
    H, W, C = cur.shape
    valid = covered.copy()
    cur = np.ascontiguousarray(cur, f32)
    for _ in range(passes):
        prev_valid, prev = valid.copy(), cur.copy()
        vpad = np.pad(prev_valid, 1)
        near = np.zeros((H, W), bool)
        for dy, dx in _LMF_RING:
            near |= vpad[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
        for y, x in np.argwhere(near & ~prev_valid):         # the pass's frontier, texel by texel: the order of the sum is the contract
            total, count = np.zeros(C, f32), 0
            for dy, dx in _LMF_RING:
                qy, qx = y + dy, x + dx
                if 0 <= qy < H and 0 <= qx < W and prev_valid[qy, qx]:
                    total = total + prev[qy, qx]
                    count += 1
            cur[y, x] = total / f32(count)
            valid[y, x] = True
    return cur, valid


def _check_finish_passes(levels, normal_power_log2, dilate):
    levels, npow, dilate = int(levels), int(normal_power_log2), int(dilate)
    if not (0 <= levels <= 8 and 0 <= npow <= 7 and 0 <= dilate <= 256):
        raise ValueError("levels must be in 0 .. 8, normal_power_log2 in 0 .. 7 and dilate in 0 .. 256")
    return levels, npow, dilate


def _lmf_finish(img, P, N, levels, normal_power_log2, sigma_plane, reach, sigma_color, dilate):
    """lightmap_finish behind its table check, for an image [H, W, C], C >= 3: the parameter checks, the levels, the dilation"""
    f32 = np.float32
    levels, npow, dilate = _check_finish_passes(levels, normal_power_log2, dilate)
    sig_p, rch, sig_c0 = f32(sigma_plane), f32(reach), f32(sigma_color)
    if not (sig_p > 0 and rch > 0 and sig_c0 > 0):
        raise ValueError("sigma_plane, reach and sigma_color must be > 0 (inf turns one off)")
    covered = _lm_covered(N)
    cur = np.where(covered[..., None], img, f32(0.0))
    with np.errstate(all="ignore"):
        for level in range(levels):
            s = 1 << level
            cur, _ = _lmf_level(cur, P, N, covered, s, npow, sig_p, rch, sig_c0 / f32(s))
        return _lmf_dilate(cur, covered, dilate)


def lightmap_finish(image, points, normals, levels: int = 3, normal_power_log2: int = 5, sigma_plane: float = float("inf"),
                    reach: float = float("inf"), sigma_color: float = float("inf"), dilate: int = 4):
    """Finish a baked lightmap on the host (numpy only): an edge-aware a-trous filter guided by the atlas's own table, then gutter
    dilation.  This is the DEFINITION of mi_lightmap_finish, which equals it bit for bit.  `image` [H, W, 3] f32 is the raw bake
    (bake_lightmap's f32 image: empty texels zero), `points` and `normals` [H, W, 3] f32 the CENTRE table of the atlas (lightmap_texels
    without jitter, also for a jittered bake).  Returns (out [H, W, 3] f32, valid [H, W] bool).
    A texel is covered when its normal is not all-zero.  Everything is f32, one rounding per operation, in the order of the building blocks above.
    Filter: levels i = 0 .. levels-1, step s = 2^i, each reading the previous level's image.  A covered texel p visits the 25 taps
    q = p + s (dx, dy), dy outer, dx inner, both -2 .. 2, skipping taps outside the image and empty ones, and those the reach test
    rejects: with D = P_q - P_p a tap other than the centre is kept only when |D|^2 <= (reach s)^2 (dx^2 + dy^2) — `reach` is the world
    length one texel step may span, a hard cut against taps that land in another chart.  Its weight is the product of the B3 kernel
    H5[dy] H5[dx], the normal weight max(0, n_p . n_q)^(2^normal_power_log2), the plane weight max(0, 1 - |n_p . D| / sigma_plane)
    and the colour weight max(0, 1 - (|dr| + |dg| + |db|) / (sigma_color / s)); the texel becomes the weighted mean.  inf turns
    sigma_plane, reach or sigma_color off.  Empty texels are +0.0.
    Dilation: `dilate` passes; in each a texel that is not valid but has valid 8-neighbours in the previous pass's state takes their
    mean (summed dy outer, dx inner) and turns valid: texel t is filled in pass number Chebyshev-distance(t, covered).
    Non-finite values spoil the texels whose footprint (radius 2 (2^levels - 1) + dilate) reaches them, and no others."""
    img, P, N = check_finish_tables(image, points, normals)
    return _lmf_finish(img, P, N, levels, normal_power_log2, sigma_plane, reach, sigma_color, dilate)


def check_finish_sh_tables(sh, points, normals):
    """(sh [H, W, 9, 3], points [H, W, 3], normals [H, W, 3]) as contiguous float32 arrays, 1 <= W, H <= 32768, for lightmap_finish_sh;
    the guides may be lightmap_texels' [1, H, W, 3]"""
    S = np.ascontiguousarray(sh, np.float32)
    P, N = (np.ascontiguousarray(_centre_table(t), np.float32) for t in (points, normals))
    if S.ndim != 4 or S.shape[2:] != (9, 3) or P.shape != S.shape[:2] + (3,) or N.shape != P.shape:
        raise ValueError(f"sh must be [H, W, 9, 3] and points and normals [H, W, 3], got {S.shape}, {P.shape} and {N.shape}")
    if not (1 <= S.shape[0] <= 32768 and 1 <= S.shape[1] <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {S.shape[1]} x {S.shape[0]}")
    return S, P, N


def lightmap_finish_sh(sh, points, normals, levels: int = 3, normal_power_log2: int = 5, sigma_plane: float = float("inf"),
                       reach: float = float("inf"), sigma_color: float = float("inf"), dilate: int = 4):
    """Finish a directional lightmap on the host (numpy only): lightmap_finish for [H, W, 9, 3] SH L2 records (bake_lightmap_sh's first
    result).  This is the DEFINITION of mi_lightmap_finish_sh, which equals it bit for bit.  Guides, levels, taps, tap order, the B3
    kernel, the normal and plane weights, the reach test, the dilation and the parameter ranges are lightmap_finish's; the colour
    distance is taken from the three k = 0 coefficients of the current level, and the one weight per tap serves all 27 channels:
    sc[j] = sc[j] + w c_q[j], then sc[j] / sw.  The dilation sums all 27 channels over the same neighbours with one count.  Empty
    texels are 27 x +0.0.  Returns (out [H, W, 9, 3] f32, valid [H, W] bool).
    Two identities follow: out[..., 0, :] is lightmap_finish of sh[..., 0, :] with the same parameters, and with sigma_color = inf
    out[..., k, :] is lightmap_finish of sh[..., k, :] for every k."""
    S, P, N = check_finish_sh_tables(sh, points, normals)
    H, W = S.shape[:2]
    out, valid = _lmf_finish(S.reshape(H, W, 27), P, N, levels, normal_power_log2, sigma_plane, reach, sigma_color, dilate)
    return np.ascontiguousarray(out.reshape(H, W, 9, 3)), valid


def check_sh_eval(sh, normals):
    """(sh [n, 9, 3] f32, normals [n, 3] f32, leading shape) for lightmap_sh_eval: sh [..., 9, 3] and normals [..., 3] with one leading
    shape (an atlas [H, W, 9, 3] with its [H, W, 3] normal table is one; lightmap_texels' [1, H, W, 3] as well).  The values are not
    looked at.  Raises ValueError."""
    S, N = np.asarray(sh, np.float32), np.asarray(normals, np.float32)
    if N.ndim == S.ndim and N.shape[0] == 1 and N.shape[1:-1] == S.shape[:-2]:
        N = N[0]
    if S.ndim < 2 or S.shape[-2:] != (9, 3) or N.ndim < 1 or N.shape[-1] != 3 or N.shape[:-1] != S.shape[:-2]:
        raise ValueError(f"sh must be [..., 9, 3] and normals [..., 3] with the same leading shape, got {S.shape} and {N.shape}")
    if N.size // 3 >= 1 << 32:
        raise ValueError(f"{N.size // 3} points exceed 2^32 - 1")
    return np.ascontiguousarray(S.reshape(-1, 9, 3)), np.ascontiguousarray(N.reshape(-1, 3)), N.shape[:-1]


def lightmap_sh_eval(sh, normals) -> np.ndarray:
    """The irradiance of a directional lightmap on the host (numpy only): E(n) of every SH L2 record `sh` [..., 9, 3] at its normal
    [..., 3].  This is the DEFINITION of mi_lightmap_sh_eval, which equals it bit for bit, and it is probe_volume_sample on a
    1 x 1 x 1 volume holding the record: all f32, (x, y, z) = n / sqrt((nx nx + ny ny) + nz nz),
    b = (1, y, z, x, x y, y z, 3 (z z) - 1, x z, x x - y y), r[k] = sh[k] * PV_K[k], e = b0 r[0] + ... + b8 r[8] left to right.
    An all-zero normal gives +0.0.  NOT clamped: SH ringing can take E slightly below zero beside strong directional light.  The
    atlas's own normals give the plain irradiance map, normal-mapped normals the detail.  Returns [..., 3] f32; divide by pi and
    multiply by the albedo for a Lambertian surface's outgoing radiance."""
    f32 = np.float32
    S, N, shape = check_sh_eval(sh, normals)
    with np.errstate(all="ignore"):
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        covered = ~((nx == 0) & (ny == 0) & (nz == 0))
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        x, y, z = nx / l, ny / l, nz / l
        b = (np.ones(len(N), f32), y, z, x, x * y, y * z, f32(3.0) * (z * z) - f32(1.0), x * z, x * x - y * y)
        r = S * PV_K[None, :, None]
        e = b[0][:, None] * r[:, 0, :]
        for k in range(1, 9):
            e = e + b[k][:, None] * r[:, k, :]
        E = np.where(covered[:, None], e, f32(0.0))
    assert E.dtype == np.float32
    return np.ascontiguousarray(E.reshape(shape + (3,)))


def check_lightmap_lookup(image, uv, valid=None, flags: int = 0, normals=None):
    """Input checking of a lightmap lookup (mi_lightmap_sample, mi_lightmap_sh_sample), no GPU needed: `image` [H, W, 3], [H, W, 27] or
    [H, W, 9, 3] with 1 <= W, H <= 32768; `uv` [..., 2]; `valid` None or [H, W] (0 = the texel takes no part: the finish calls' valid as
    it stands); `normals` None or [..., 3] with uv's leading shape; flags 0 or abi.MI_LS_NEAREST.  The values are not looked at.  Returns
    (image [H, W, C] f32, uv [n, 2] f32, valid [H, W] uint8 or None, flags, normals [n, 3] f32 or None, leading shape), all contiguous;
    raises ValueError."""
    img = np.asarray(image, np.float32)
    if img.ndim == 4 and img.shape[2:] == (9, 3):
        img = img.reshape(img.shape[:2] + (27,))
    if img.ndim != 3 or img.shape[2] not in (3, 27):
        raise ValueError(f"image must be [H, W, 3], [H, W, 27] or [H, W, 9, 3], got {np.shape(image)}")
    H, W = img.shape[:2]
    if not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {W} x {H}")
    flags = int(flags)
    if flags & ~abi.MI_LS_NEAREST:
        raise ValueError(f"unknown flag bits {flags & ~abi.MI_LS_NEAREST:#x}")
    T = np.asarray(uv, np.float32)
    if T.ndim < 1 or T.shape[-1] != 2:
        raise ValueError(f"uv must be [..., 2], got {T.shape}")
    if T.size // 2 >= 1 << 32:
        raise ValueError(f"{T.size // 2} points exceed 2^32 - 1")
    v8 = None
    if valid is not None:
        v8 = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        if v8.shape != (H, W):
            raise ValueError(f"valid must be [{H}, {W}], got {v8.shape}")
    N = None
    if normals is not None:
        N = np.asarray(normals, np.float32)
        if N.ndim < 1 or N.shape[-1] != 3 or N.shape[:-1] != T.shape[:-1]:
            raise ValueError(f"normals must be [..., 3] with uv's leading shape, got {N.shape} for uv {T.shape}")
        N = np.ascontiguousarray(N.reshape(-1, 3))
    return np.ascontiguousarray(img), np.ascontiguousarray(T.reshape(-1, 2)), v8, flags, N, T.shape[:-1]


# The building blocks of lightmap_sample and lightmap_sh_sample: each rule of those definitions is written once, here.  All f32, one
# rounding per operation, in the order written; the callers hold np.errstate(all="ignore").
_LML_TAPS = ((0, 0), (0, 1), (1, 0), (1, 1))                      # (dy, dx): dy outer, dx inner


def _lml_axis(t, n):
    """One axis of the bilinear form at coordinate t in 0 .. 1 of n texels: ((i0, i1), (1 - f, f)).  probe_volume_sample's index
    expressions; fmax sends a NaN to 0, so the indices stay in range for any t."""
    f32 = np.float32
    g = t * f32(n) - f32(0.5)
    g = np.fmin(np.fmax(g, f32(0.0)), f32(n - 1))
    i0 = np.minimum(np.floor(g).astype(np.int64), max(n - 2, 0))
    f = g - i0.astype(f32)
    return (i0, np.minimum(i0 + 1, n - 1)), (f32(1.0) - f, f)


def _lml_unit(t):
    """The reference's clamp of a texture coordinate (texture.rs:28-29); a NaN leaves it as 0"""
    return np.fmin(np.fmax(t, np.float32(0.0)), np.float32(0.999))


def _lml_texel(s, n, nan):
    """The texel of the clamped coordinate s (or of its mirror 1 - s) among n: trunc(s n), at most n - 1; 0 where the coordinate was a
    NaN (`nan`), as Rust's saturating cast gives"""
    return np.where(nan, 0, np.minimum(np.trunc(s * np.float32(n)).astype(np.int64), n - 1))


def _lml_lookup(img, ok, uv, flags, value, channels):
    """The lookup both definitions share: `value` turns the texels [n, C] gathered for one tap into what is interpolated [n, channels].
    Returns (out [n, channels] f32, weight [n] f32)."""
    f32 = np.float32
    zero, one = f32(0.0), f32(1.0)
    H, W = img.shape[:2]
    u, v = uv[:, 0], uv[:, 1]
    if flags & abi.MI_LS_NEAREST:
        x = _lml_texel(_lml_unit(u), W, np.isnan(u))
        y = _lml_texel(one - _lml_unit(v), H, np.isnan(v))
        take = ok[y, x]
        return np.where(take[:, None], value(img[y, x]), zero), np.where(take, one, zero)
    ix, wx = _lml_axis(u, W)
    iy, wy = _lml_axis(one - v, H)
    acc = np.zeros((len(uv), channels), f32)
    sw = np.zeros(len(uv), f32)
    for dy, dx in _LML_TAPS:
        yi, xi = iy[dy], ix[dx]
        w = wx[dx] * wy[dy]
        take = (w > 0) & ok[yi, xi]                      # a tap that does not take part is not read: its texel may hold anything
        acc = np.where(take[:, None], acc + w[:, None] * value(img[yi, xi]), acc)
        sw = np.where(take, sw + w, sw)
    return np.where((sw > 0)[:, None], acc / sw[:, None], zero), sw


def lightmap_sample(image, uv, valid=None, flags: int = 0):
    """Read a finished lightmap at uv points on the host (numpy only).  This is the DEFINITION of mi_lightmap_sample, which equals it bit
    for bit.  Arguments as check_lightmap_lookup.  Returns (out [..., C] f32, weight [...] f32), C = 3 or 27.
    Everything is f32, one rounding per operation (+ - * /, floor, fmin, fmax), in the order written in the blocks above.
    Bilinear (flags == 0): gx = u W - 0.5, gy = (1 - v) H - 0.5 (row 0 is v = 1: Texture::sample's flip, texture.rs:29); per axis
    g = fmin(fmax(g, 0), n - 1), i0 = min(floor(g), max(n - 2, 0)), f = g - i0, i1 = min(i0 + 1, n - 1) — probe_volume_sample's index
    expressions, the clamp wrap mode.  Four taps, dy outer, dx inner: w = w_x[dx] w_y[dy] with w_a = (1 - f, f); a tap takes part when
    w > 0 and its texel is valid, and one that does not is not read.  acc += w t, sw += w from +0; out = acc / sw when sw > 0, else +0;
    weight = sw.  At a texel centre the result is the texel as a number (a -0 comes back +0).
    MI_LS_NEAREST: the reference's own addressing (texture.rs:28-29), x = min(trunc(fmin(fmax(u, 0), 0.999) W), W - 1) and
    y = min(trunc((1 - fmin(fmax(v, 0), 0.999)) H), H - 1), 0 for a NaN coordinate: the texel as it stands with weight 1, +0 with weight 0
    when it is invalid.
    Non-finite uv or texels spoil only the points whose taking-part taps touch them."""
    img, T, v8, flags, _, shape = check_lightmap_lookup(image, uv, valid, flags)
    ok = np.ones(img.shape[:2], bool) if v8 is None else v8 != 0
    with np.errstate(all="ignore"):
        out, sw = _lml_lookup(img, ok, T, flags, lambda t: t, img.shape[2])
    assert out.dtype == np.float32 and sw.dtype == np.float32
    return np.ascontiguousarray(out.reshape(shape + (img.shape[2],))), np.ascontiguousarray(sw.reshape(shape))


def lightmap_sh_sample(sh, uv, normals, valid=None, flags: int = 0):
    """The irradiance of a finished directional lightmap at uv points and their normals on the host (numpy only): lightmap_sample and
    lightmap_sh_eval in one pass.  This is the DEFINITION of mi_lightmap_sh_sample, which equals it bit for bit.  `sh` [H, W, 9, 3] (or
    flat [H, W, 27]); the other arguments as check_lightmap_lookup.  Returns (E [..., 3] f32, weight [...] f32).
    An all-zero normal (either sign of zero) gives +0 and weight 0.  Otherwise x, y, z, b and PV_K are lightmap_sh_eval's, the taps and
    their weights lightmap_sample's; per tap that takes part e = b0 (sh[0] K0) + ... + b8 (sh[8] K8) left to right, acc += w e,
    sw += w, E = acc / sw: probe_volume_sample's order, never an interpolated record.  With MI_LS_NEAREST E is e of the one texel:
    lightmap_sh_eval of that record, bit for bit.  NOT bit-equal to lightmap_sample of the 27 channels followed by lightmap_sh_eval."""
    f32 = np.float32
    if normals is None:
        raise ValueError("normals are required")
    img, T, v8, flags, N, shape = check_lightmap_lookup(sh, uv, valid, flags, normals)
    if img.shape[2] != 27:
        raise ValueError(f"sh must be [H, W, 9, 3] or [H, W, 27], got {np.shape(sh)}")
    ok = np.ones(img.shape[:2], bool) if v8 is None else v8 != 0
    with np.errstate(all="ignore"):
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        covered = _lm_covered(N)
        l = np.sqrt((nx * nx + ny * ny) + nz * nz)
        x, y, z = nx / l, ny / l, nz / l
        b = (np.ones(len(N), f32), y, z, x, x * y, y * z, f32(3.0) * (z * z) - f32(1.0), x * z, x * x - y * y)

        def value(t):
            r = t.reshape(-1, 9, 3) * PV_K[None, :, None]
            e = b[0][:, None] * r[:, 0, :]
            for k in range(1, 9):
                e = e + b[k][:, None] * r[:, k, :]
            return e
        E, sw = _lml_lookup(img, ok, T, flags, value, 3)
        E = np.where(covered[:, None], E, f32(0.0))
        sw = np.where(covered, sw, f32(0.0))
    assert E.dtype == np.float32 and sw.dtype == np.float32
    return np.ascontiguousarray(E.reshape(shape + (3,))), np.ascontiguousarray(sw.reshape(shape))


# ---- lightmap mips: the coverage-aware pyramid of a finished lightmap and the trilinear lookup that reads it ----
# The layout rule, written once: level l of a W x H image is _lmm_extent(W, l) x _lmm_extent(H, l) (ceil halving), the full chain has
# _lmm_full(W, H) levels, and levels 1 .. L - 1 lie tightly one after the other in one buffer.
_LMM_CHILDREN = ((0, 0), (0, 1), (1, 0), (1, 1))                  # (dy, dx): dy outer, dx inner


def _lmm_extent(n, l):
    """The extent of level l of an axis of n texels: ceil(n / 2^l), so that texel x of level l covers the level-0 texels
    [x 2^l, (x + 1) 2^l) that lie inside the image"""
    return (n + (1 << l) - 1) >> l


def _lmm_full(W, H):
    """The number of levels of the full chain, level 0 counted: 1 + ceil(log2(max(W, H))); its last level is 1 x 1"""
    return 1 + (max(W, H) - 1).bit_length()


def lightmap_mip_layout(width: int, height: int, levels: int = 0):
    """The layout of a lightmap's mip chain, no GPU needed (render_plan.cpp mip_plan is the same rule): [(W_l, H_l, offset_l)] for
    l = 0 .. L - 1.  `levels` counts level 0; 0 means the full chain, 1 + ceil(log2(max(W, H))) levels; more than that is refused.
    W_l = (W + 2^l - 1) >> l and H_l likewise.  offset_l is where level l starts, in texels, in the buffers that hold levels
    1 .. L - 1 tightly one after the other (mips [sum W_l H_l][C] f32, mip_valid u8 and mip_coverage f32 [sum W_l H_l]): the running sum
    from level 1 on.  Level 0 is the image itself and is not copied: its offset is given as 0.  Raises ValueError."""
    W, H, levels = int(width), int(height), int(levels)
    if not (1 <= W <= 32768 and 1 <= H <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {W} x {H}")
    if not (0 <= levels <= _lmm_full(W, H)):
        raise ValueError(f"levels {levels} is not in 0 .. {_lmm_full(W, H)}, the full chain of {W} x {H}")
    out, off = [], 0
    for l in range(levels or _lmm_full(W, H)):
        wl, hl = _lmm_extent(W, l), _lmm_extent(H, l)
        out.append((wl, hl, off))
        off += wl * hl if l else 0
    return out


def check_lightmap_mips(image, valid=None, levels: int = 0):
    """Input checking of mi_lightmap_mips, no GPU needed: `image` [H, W, 3], [H, W, 27] or [H, W, 9, 3] with 1 <= W, H <= 32768; `valid`
    None or [H, W] (0 = the texel takes no part); `levels` 0 (the full chain) or at most the full chain.  The values are not looked at.
    Returns (image [H, W, C] f32, valid [H, W] uint8 or None, the layout of lightmap_mip_layout); raises ValueError."""
    img = np.asarray(image, np.float32)
    if img.ndim == 4 and img.shape[2:] == (9, 3):
        img = img.reshape(img.shape[:2] + (27,))
    if img.ndim != 3 or img.shape[2] not in (3, 27):
        raise ValueError(f"image must be [H, W, 3], [H, W, 27] or [H, W, 9, 3], got {np.shape(image)}")
    H, W = img.shape[:2]
    layout = lightmap_mip_layout(W, H, levels)
    v8 = None
    if valid is not None:
        v8 = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        if v8.shape != (H, W):
            raise ValueError(f"valid must be [{H}, {W}], got {v8.shape}")
    return np.ascontiguousarray(img), v8, layout


def _lmm_level(prev, cov, Wn, Hn):
    """One level of the pyramid from the one before: prev [Hp, Wp, C] f32 and its coverage cov [Hp, Wp] f32 to
    (out [Hn, Wn, C] f32, coverage [Hn, Wn] f32).  The rule of lightmap_mips, written once."""
    f32 = np.float32
    Hp, Wp, C = prev.shape
    y, x = np.mgrid[0:Hn, 0:Wn]
    acc = np.zeros((Hn, Wn, C), f32)
    sc = np.zeros((Hn, Wn), f32)
    for dy, dx in _LMM_CHILDREN:
        cy, cx = 2 * y + dy, 2 * x + dx
        inside = (cy < Hp) & (cx < Wp)
        yi, xi = np.minimum(cy, Hp - 1), np.minimum(cx, Wp - 1)          # (an address for the gather: what lies outside takes no part)
        c = cov[yi, xi]
        take = inside & (c > 0)                    # a child that takes no part is not read: its texel may hold anything
        acc = np.where(take[..., None], acc + c[..., None] * prev[yi, xi], acc)
        sc = np.where(take, sc + c, sc)
    return np.where((sc > 0)[..., None], acc / sc[..., None], f32(0.0)), sc * f32(0.25)


def lightmap_mips(image, valid=None, levels: int = 0):
    """The coverage-aware mip chain of a finished lightmap on the host (numpy only).  This is the DEFINITION of mi_lightmap_mips, which
    equals it bit for bit.  Arguments as check_lightmap_mips.  Returns (mips, valids, coverage): three lists with one array per level
    l = 0 .. L - 1, [H_l, W_l, C] f32, [H_l, W_l] uint8 and [H_l, W_l] f32, sizes as lightmap_mip_layout; level 0 is the image itself,
    its mask (all ones for None) and cov_0 = 1.0 where valid, else 0.0.
    Everything is f32, one rounding per operation, in the order written.  For l >= 1 texel (x, y) has the children (2y + dy, 2x + dx) of
    level l - 1, dy outer, dx inner; a child takes part when it lies inside level l - 1 and its c = cov_(l-1) > 0, and one that does not
    is not read.  acc = acc + c t and sc = sc + c from +0; out = acc / sc when sc > 0, else +0; cov_l = sc * 0.25; valid_l = cov_l > 0.
    So cov_l is the fraction of the texel's level-0 footprint that is valid (exact while 4^l <= 2^24, l <= 12; rounded as written
    beyond) and out the mean over exactly those texels.  Texels behind valid == 0 may hold anything; a non-finite valid texel spoils
    only its own ancestors."""
    img, v8, layout = check_lightmap_mips(image, valid, levels)
    f32 = np.float32
    ok = np.ones(img.shape[:2], bool) if v8 is None else v8 != 0
    mips, valids, covs = [img], [ok.astype(np.uint8)], [np.where(ok, f32(1.0), f32(0.0))]
    with np.errstate(all="ignore"):
        for wl, hl, _ in layout[1:]:
            out, cov = _lmm_level(mips[-1], covs[-1], wl, hl)
            assert out.dtype == np.float32 and cov.dtype == np.float32
            mips.append(np.ascontiguousarray(out))
            covs.append(np.ascontiguousarray(cov))
            valids.append((cov > 0).astype(np.uint8))
    return mips, valids, covs


def _lmm_pack(chain, dtype, tail=()):
    """Levels 1 .. L - 1 of a per-level list as the one tight buffer the C calls take (at least one element long)"""
    flat = [np.asarray(a, dtype).reshape((-1,) + tuple(tail)) for a in chain[1:]]
    return np.ascontiguousarray(np.concatenate(flat)) if flat else np.zeros((1,) + tuple(tail), dtype)


def check_lightmap_lod(chain, uv, lod, valid_chain=None, flags: int = 0, normals=None):
    """Input checking of the trilinear lookups (mi_lightmap_sample_lod, mi_lightmap_sh_sample_lod), no GPU needed.  `chain` is the list
    lightmap_mips returns first: level 0 ([H, W, 3], [H, W, 27] or [H, W, 9, 3], 1 <= W, H <= 32768) and levels 1 .. L - 1 of
    lightmap_mip_layout's sizes, L at most the full chain.  `valid_chain` is None (everything valid) or a list of L masks of the
    levels' sizes; entry 0 may be None, and entries 1 .. L - 1 are either all None or all given.  `uv` [..., 2]; `lod` a scalar or uv's
    leading shape; `normals` None or [..., 3] with uv's leading shape; `flags` must be 0: abi.MI_LS_NEAREST is refused (nearest
    addressing is the reference's, and the reference has no mips).  The values are not looked at.  Returns (levels [L] of [H_l, W_l, C]
    f32, masks [L] of bool [H_l, W_l] or None, uv [n, 2] f32, lod [n] f32, normals [n, 3] f32 or None, leading shape); raises
    ValueError."""
    if not isinstance(chain, (list, tuple)) or len(chain) == 0:
        raise ValueError("chain must be a list of levels, level 0 first")
    flags = int(flags)
    if flags & abi.MI_LS_NEAREST:
        raise ValueError("MI_LS_NEAREST is refused: the reference's nearest addressing has no mips")
    if flags:
        raise ValueError(f"unknown flag bits {flags:#x}")
    img, T, _, _, N, shape = check_lightmap_lookup(chain[0], uv, None, 0, normals)
    H, W, ch = img.shape
    if len(chain) > _lmm_full(W, H):
        raise ValueError(f"{len(chain)} levels are more than the full chain of {W} x {H}, {_lmm_full(W, H)}")
    layout = lightmap_mip_layout(W, H, len(chain))
    levels = [img]
    for l in range(1, len(chain)):
        a = np.asarray(chain[l], np.float32)
        wl, hl, _ = layout[l]
        if a.shape[:2] != (hl, wl) or a.size != hl * wl * ch:
            raise ValueError(f"level {l} must be [{hl}, {wl}, {ch}], got {a.shape}")
        levels.append(np.ascontiguousarray(a.reshape(hl, wl, ch)))
    masks = [None] * len(chain)
    if valid_chain is not None:
        if not isinstance(valid_chain, (list, tuple)) or len(valid_chain) != len(chain):
            raise ValueError(f"valid_chain must be None or a list of {len(chain)} masks")
        given = [v is not None for v in valid_chain[1:]]
        if any(given) and not all(given):
            raise ValueError("the masks of levels 1 .. L - 1 are either all None or all given")
        for l, v in enumerate(valid_chain):
            if v is None:
                continue
            wl, hl, _ = layout[l]
            m = np.asarray(v) != 0
            if m.shape != (hl, wl):
                raise ValueError(f"mask {l} must be [{hl}, {wl}], got {m.shape}")
            masks[l] = np.ascontiguousarray(m)
    D = np.asarray(lod, np.float32)
    if D.ndim and D.shape != shape:
        raise ValueError(f"lod must be a scalar or {shape}, got {D.shape}")
    D = np.ascontiguousarray(np.broadcast_to(D, shape).reshape(-1))
    return levels, masks, T, D, N, shape


def _lml_axis_lod(t, n0, s, n):
    """One axis of the bilinear form at level l: coordinate t in 0 .. 1, n0 texels at level 0, s = 2^-l (exact), n texels at level l:
    ((i0, i1), (1 - f, f)).  _lml_axis' clamp and index expressions; at l = 0 this is _lml_axis itself."""
    f32 = np.float32
    g = (t * f32(n0)) * s - f32(0.5)
    g = np.fmin(np.fmax(g, f32(0.0)), f32(n - 1))
    i0 = np.minimum(np.floor(g).astype(np.int64), max(n - 2, 0))
    f = g - i0.astype(f32)
    return (i0, np.minimum(i0 + 1, n - 1)), (f32(1.0) - f, f)


def _lml_levels(lod, L):
    """The two levels a point reads among L and their weights: ((l_a, l_b), (1 - f, f)).  fmax sends a NaN to 0."""
    f32 = np.float32
    lam = np.fmin(np.fmax(lod, f32(0.0)), f32(L - 1))
    la = np.minimum(np.floor(lam).astype(np.int64), max(L - 2, 0))
    fl = lam - la.astype(f32)
    return (la, np.minimum(la + 1, L - 1)), (f32(1.0) - fl, fl)


def _lml_lookup_lod(levels, oks, uv, lod, value, channels):
    """The trilinear lookup both _lod definitions share: `value(t, at)` turns the texels [m, C] gathered for one tap of the points `at`
    into what is interpolated [m, channels].  Returns (out [n, channels] f32, weight [n] f32)."""
    f32 = np.float32
    zero, one = f32(0.0), f32(1.0)
    H0, W0 = levels[0].shape[:2]
    u, v = uv[:, 0], uv[:, 1]
    lv, wl = _lml_levels(lod, len(levels))
    acc = np.zeros((len(uv), channels), f32)
    sw = np.zeros(len(uv), f32)
    for side in (0, 1):                                  # level a, then level b
        for l, img in enumerate(levels):
            at = np.nonzero((lv[side] == l) & (wl[side] > 0))[0]        # a level whose weight is not > 0 takes no part
            if len(at) == 0:
                continue
            H, W = img.shape[:2]
            s = f32(2.0 ** -l)
            ix, wx = _lml_axis_lod(u[at], W0, s, W)
            iy, wy = _lml_axis_lod(one - v[at], H0, s, H)
            a, b = acc[at], sw[at]
            for dy, dx in _LML_TAPS:
                yi, xi = iy[dy], ix[dx]
                w = wl[side][at] * (wx[dx] * wy[dy])
                take = (w > 0) & oks[l][yi, xi]            # a tap that does not take part is not read
                a = np.where(take[:, None], a + w[:, None] * value(img[yi, xi], at), a)
                b = np.where(take, b + w, b)
            acc[at], sw[at] = a, b
    return np.where((sw > 0)[:, None], acc / sw[:, None], zero), sw


def lightmap_sample_lod(chain, uv, lod, valid_chain=None, flags: int = 0):
    """Read a lightmap's mip chain at uv points and levels of detail on the host (numpy only): trilinear over the valid texels.  This
    is the DEFINITION of mi_lightmap_sample_lod, which equals it bit for bit.  Arguments as check_lightmap_lod (`chain`, `valid_chain`:
    lightmap_mips' first two results).  Returns (out [..., C] f32, weight [...] f32).
    Everything is f32, one rounding per operation, in the order written.  With L levels: lam = fmin(fmax(lod, 0), L - 1) (a NaN becomes
    0), l_a = min(floor(lam), max(L - 2, 0)), f = lam - l_a, l_b = min(l_a + 1, L - 1); the level weights are (1 - f, f), and a level
    whose weight is not > 0 takes no part and is not read.  Per level l that takes part and per axis g = (t n_0) 2^-l - 0.5 (t = u, or
    1 - v), then lightmap_sample's clamp and index expressions with n_l; the scaling is exact, and at l = 0 this is lightmap_sample's
    expression.  Taps: level a then level b, each dy outer, dx inner; w = w_level (w_x[dx] w_y[dy]); a tap takes part when w > 0 and its
    texel is valid at its level.  One acc and one sw over the up to eight taps; out = acc / sw when sw > 0, else +0; weight = sw.
    With one level, lod <= 0 or a NaN lod the result is lightmap_sample of level 0, bit for bit; at an integer lod = l on a size
    divisible by 2^l it is lightmap_sample of level l with that level's mask."""
    levels, masks, T, D, _, shape = check_lightmap_lod(chain, uv, lod, valid_chain, flags)
    oks = [np.ones(a.shape[:2], bool) if m is None else m for a, m in zip(levels, masks)]
    ch = levels[0].shape[2]
    with np.errstate(all="ignore"):
        out, sw = _lml_lookup_lod(levels, oks, T, D, lambda t, at: t, ch)
    assert out.dtype == np.float32 and sw.dtype == np.float32
    return np.ascontiguousarray(out.reshape(shape + (ch,))), np.ascontiguousarray(sw.reshape(shape))


def lightmap_sh_sample_lod(chain, uv, normals, lod, valid_chain=None, flags: int = 0):
    """The irradiance of a directional lightmap's mip chain at uv points, their normals and levels of detail on the host (numpy only).
    This is the DEFINITION of mi_lightmap_sh_sample_lod, which equals it bit for bit.  `chain` holds [H_l, W_l, 9, 3] (or flat 27)
    records; the other arguments as check_lightmap_lod.  Returns (E [..., 3] f32, weight [...] f32).
    An all-zero normal (either sign of zero) gives +0 and weight 0.  Otherwise the levels, taps and weights are lightmap_sample_lod's
    and each tap's record becomes e as in lightmap_sh_sample before it is weighted: three accumulators, never an interpolated
    record.  With one level, lod <= 0 or a NaN lod the result is lightmap_sh_sample of level 0, bit for bit."""
    f32 = np.float32
    if normals is None:
        raise ValueError("normals are required")
    levels, masks, T, D, N, shape = check_lightmap_lod(chain, uv, lod, valid_chain, flags, normals)
    if levels[0].shape[2] != 27:
        raise ValueError(f"the levels must be [H, W, 9, 3] or [H, W, 27], got {np.shape(chain[0])}")
    oks = [np.ones(a.shape[:2], bool) if m is None else m for a, m in zip(levels, masks)]
    with np.errstate(all="ignore"):
        nx, ny, nz = N[:, 0], N[:, 1], N[:, 2]
        covered = _lm_covered(N)
        ln = np.sqrt((nx * nx + ny * ny) + nz * nz)
        x, y, z = nx / ln, ny / ln, nz / ln
        b = (np.ones(len(N), f32), y, z, x, x * y, y * z, f32(3.0) * (z * z) - f32(1.0), x * z, x * x - y * y)

        def value(t, at):
            r = t.reshape(-1, 9, 3) * PV_K[None, :, None]
            e = b[0][at][:, None] * r[:, 0, :]
            for k in range(1, 9):
                e = e + b[k][at][:, None] * r[:, k, :]
            return e
        E, sw = _lml_lookup_lod(levels, oks, T, D, value, 3)
        E = np.where(covered[:, None], E, f32(0.0))
        sw = np.where(covered, sw, f32(0.0))
    assert E.dtype == np.float32 and sw.dtype == np.float32
    return np.ascontiguousarray(E.reshape(shape + (3,))), np.ascontiguousarray(sw.reshape(shape))


# ---- packed lightmaps: f16 and RGB9E5 storage (mi_lightmap_pack, mi_lightmap_unpack, mi_lightmap_*_packed) ----
# Both formats decode to f32 exactly, so a packed lookup IS the f32 lookup of the unpacked texels; the only arithmetic of their own is
# in the two encoders below.

def _check_packed_format(format, channels=None, sh: bool = False) -> int:
    """What every packed call checks of its format: abi.MI_LP_F16 (3 or 27 channels) or abi.MI_LP_RGB9E5 (3 channels, not the SH
    form); 0, the f32 of the unpacked calls, is refused.  Returns the format; raises ValueError."""
    fmt = int(format)
    if fmt not in (abi.MI_LP_F16, abi.MI_LP_RGB9E5):
        raise ValueError(f"format {format} is not MI_LP_F16 or MI_LP_RGB9E5 (f32 texels take the unpacked calls)")
    if sh and fmt != abi.MI_LP_F16:
        raise ValueError("SH coefficients are signed: only MI_LP_F16 holds them")
    if channels is not None:
        if channels not in (3, 27):
            raise ValueError(f"channels must be 3 or 27, got {channels}")
        if fmt == abi.MI_LP_RGB9E5 and channels != 3:
            raise ValueError(f"MI_LP_RGB9E5 holds 3 unsigned channels, not {channels} (SH records pack as MI_LP_F16)")
    return fmt


def _check_packed_array(packed, format):
    """Packed texels are uint16 [..., 3 or 27] (abi.MI_LP_F16) or uint32 [...] (abi.MI_LP_RGB9E5).  Returns (format, contiguous array)."""
    fmt = _check_packed_format(format)
    p = np.ascontiguousarray(packed)
    if fmt == abi.MI_LP_F16 and (p.dtype != np.uint16 or p.ndim < 1 or p.shape[-1] not in (3, 27)):
        raise ValueError(f"MI_LP_F16 texels must be uint16 [..., 3] or [..., 27], got {p.dtype} {p.shape}")
    if fmt == abi.MI_LP_RGB9E5 and p.dtype != np.uint32:
        raise ValueError(f"MI_LP_RGB9E5 texels must be uint32, got {p.dtype}")
    return fmt, p


def _pow2_f32(e):
    """2^e as an exact f32 built from its exponent field, -126 <= e <= 127 (an integer array)"""
    return ((np.asarray(e, np.int64) + 127).astype(np.uint32) << np.uint32(23)).view(np.float32)


def lightmap_pack(texels, format):
    """Pack f32 lightmap texels on the host (numpy only).  This is the DEFINITION of mi_lightmap_pack, which equals it bit for bit.
    `texels` [..., C] f32 with C = 3 or 27 (an [..., 9, 3] table of SH records packs to the same bytes); any leading shape: a level, a
    whole mips buffer, a list of texels.  Returns uint16 [..., C] bit patterns for abi.MI_LP_F16 (not np.float16, so NaNs compare) or
    uint32 [...] for abi.MI_LP_RGB9E5 (C = 3 only).
    f16, per float x: a NaN gives 0x7E00 (a select, not a conversion); otherwise c = fmin(fmax(x, -65504), 65504) converted
    round-to-nearest-even to binary16.  Subnormal results and the sign of zero are kept; infinities and everything beyond +-65504 become
    0x7BFF / 0xFBFF, so no infinity is ever written.
    RGB9E5 (N = 9, B = 15, largest value 65408), all f32, one rounding per operation: per channel c = 0 for a NaN, else
    fmin(fmax(x, 0), 65408); m = max(c_r, c_g, c_b); eb = ((bits(m) >> 23) & 255) - 127 (floor(log2 m); -127 for a zero or subnormal m);
    ep = max(eb, -16) + 16; ms = floor(m 2^(24 - ep) + 0.5); e = ep + (ms == 512); q_k = floor(c_k 2^(24 - e) + 0.5);
    word = q_r | q_g << 9 | q_b << 18 | e << 27.  The products are exact; the one rounding per channel is the + 0.5, so 0.5 - 2^-25
    scaled rounds up: that is the definition."""
    f32 = np.float32
    x = np.asarray(texels, f32)
    if x.ndim < 1 or x.shape[-1] not in (3, 27):
        raise ValueError(f"texels must be [..., 3] or [..., 27], got {x.shape}")
    fmt = _check_packed_format(format, x.shape[-1])
    with np.errstate(all="ignore"):
        if fmt == abi.MI_LP_F16:
            c = np.fmin(np.fmax(x, f32(-65504.0)), f32(65504.0))
            bits = c.astype(np.float16).view(np.uint16)
            return np.ascontiguousarray(np.where(x != x, np.uint16(0x7E00), bits))
        c = np.where(x != x, f32(0.0), np.fmin(np.fmax(x, f32(0.0)), f32(65408.0)))
        m = np.fmax(np.fmax(c[..., 0], c[..., 1]), c[..., 2])
        eb = ((np.ascontiguousarray(m).view(np.uint32) >> np.uint32(23)) & np.uint32(255)).astype(np.int64) - 127
        ep = np.maximum(eb, -16) + 16
        ms = np.floor(m * _pow2_f32(24 - ep) + f32(0.5))
        e = ep + (ms == f32(512.0))
        q = np.floor(c * _pow2_f32(24 - e)[..., None] + f32(0.5)).astype(np.uint32)
        assert ms.dtype == f32
    word = q[..., 0] | q[..., 1] << np.uint32(9) | q[..., 2] << np.uint32(18) | e.astype(np.uint32) << np.uint32(27)
    return np.ascontiguousarray(word).reshape(x.shape[:-1])


def lightmap_unpack(packed, format):
    """Unpack packed lightmap texels on the host (numpy only).  This is the DEFINITION of mi_lightmap_unpack; both decodes are exact.
    abi.MI_LP_F16: `packed` uint16 [..., C] (C = 3 or 27) gives f32 [..., C], the binary16 -> f32 widening.  abi.MI_LP_RGB9E5: uint32
    [...] gives f32 [..., 3], (float)q_k 2^(e - 24)."""
    fmt, p = _check_packed_array(packed, format)
    if fmt == abi.MI_LP_F16:
        return p.view(np.float16).astype(np.float32)
    s = _pow2_f32((p >> np.uint32(27)).astype(np.int64) - 24)
    q = np.stack([(p >> np.uint32(9 * k)) & np.uint32(511) for k in range(3)], axis=-1)
    return np.ascontiguousarray(q.astype(np.float32) * s[..., None])


def check_lightmap_packed(packed_chain, format, uv, lod=None, valid_chain=None, flags: int = 0, normals=None, sh: bool = False):
    """Input checking of the packed lookups (mi_lightmap_sample_packed; with sh: mi_lightmap_sh_sample_packed), no GPU needed.
    `packed_chain` is a list of packed levels as lightmap_pack returns them (uint16 [H_l, W_l, C] or uint32 [H_l, W_l]), level 0 first,
    or one such array; `format` abi.MI_LP_F16 or abi.MI_LP_RGB9E5 (3 channels, never the SH form).  With `lod` the rest is checked as
    check_lightmap_lod checks it; with lod None as check_lightmap_lookup does (abi.MI_LS_NEAREST allowed), and then there must be one
    level alone.  Returns (packed levels [L] contiguous, what the f32 check returned for the unpacked levels); raises ValueError where
    the C calls refuse."""
    fmt = _check_packed_format(format, None, sh)
    chain = list(packed_chain) if isinstance(packed_chain, (list, tuple)) else [packed_chain]
    if len(chain) == 0:
        raise ValueError("packed_chain must hold level 0")
    packed = [np.ascontiguousarray(p) for p in chain]
    levels = [lightmap_unpack(p, fmt) for p in packed]
    if levels[0].ndim == 4 and levels[0].shape[2:] == (9, 3) and fmt == abi.MI_LP_F16:
        levels = [a.reshape(a.shape[:2] + (27,)) for a in levels]
        packed = [p.reshape(p.shape[:2] + (27,)) for p in packed]
    if sh and (levels[0].ndim != 3 or levels[0].shape[2] != 27):
        raise ValueError(f"the levels must be [H, W, 9, 3] or [H, W, 27], got {np.shape(chain[0])}")
    if sh and normals is None:
        raise ValueError("normals are required")
    return packed, _check_level_form(levels, uv, lod, valid_chain, flags, normals)


def _check_level_form(levels, uv, lod, valid_chain, flags, normals=None):
    """The f32 check of a lookup that has both level forms: with `lod` check_lightmap_lod's of the chain; with lod None
    check_lightmap_lookup's of level 0, which must then be the one level given"""
    if lod is not None:
        return check_lightmap_lod(levels, uv, lod, valid_chain, flags, normals)
    if len(levels) != 1:
        raise ValueError(f"lod None reads level 0 alone: {len(levels)} levels were given")
    if isinstance(valid_chain, (list, tuple)):
        if len(valid_chain) != 1:
            raise ValueError("lod None reads level 0 alone: valid_chain must be None, one mask or a list of one")
        valid_chain = valid_chain[0]
    return check_lightmap_lookup(levels[0], uv, valid_chain, flags, normals)


def _sample_level_form(checked, lod, sh: bool = False):
    """The definition's result for what _check_level_form returned: the level-0 lookup or the trilinear one, plain or fused SH"""
    if lod is None:
        img, T, v8, flags, N, shape = checked
        out, sw = lightmap_sh_sample(img, T, N, v8, flags) if sh else lightmap_sample(img, T, v8, flags)
    else:
        levels, masks, T, D, N, shape = checked                     # (the flags are 0 here: the check refuses every other value)
        out, sw = lightmap_sh_sample_lod(levels, T, N, D, masks) if sh else lightmap_sample_lod(levels, T, D, masks)
    return out.reshape(shape + out.shape[-1:]), sw.reshape(shape)


def lightmap_sample_packed(packed_chain, format, uv, lod=None, valid_chain=None, flags: int = 0):
    """Read a packed lightmap at uv points on the host (numpy only).  This is the DEFINITION of mi_lightmap_sample_packed: unpack, then
    lightmap_sample_lod — or, with lod None, lightmap_sample of the one level (abi.MI_LS_NEAREST then gives the decoded texel as it
    stands, a -0.0 included).  Arguments as check_lightmap_packed.  Returns (out [..., C] f32, weight [...] f32)."""
    return _sample_level_form(check_lightmap_packed(packed_chain, format, uv, lod, valid_chain, flags)[1], lod)


def lightmap_sh_sample_packed(packed_chain, format, uv, normals, lod=None, valid_chain=None, flags: int = 0):
    """The irradiance of a packed directional lightmap at uv points and their normals on the host (numpy only).  This is the DEFINITION
    of mi_lightmap_sh_sample_packed: unpack (abi.MI_LP_F16 only), then lightmap_sh_sample_lod — or, with lod None, lightmap_sh_sample
    of the one level.  Returns (E [..., 3] f32, weight [...] f32)."""
    return _sample_level_form(check_lightmap_packed(packed_chain, format, uv, lod, valid_chain, flags, normals, sh=True)[1], lod, True)


# ---- BC6H lightmaps: a block encoder, the decoder, lookups that read blocks (mi_lightmap_bc6h_encode, _decode, mi_lightmap_sample_bc6h) ----
# BC6H_UF16, 3 channels, ONE block mode: the one-region mode with two 10-bit direct endpoints and 4-bit indices ("mode 11", low five bits
# 3).  A block is 16 bytes, a little-endian 128-bit integer: bits 0-4 hold 3; six 10-bit fields rw, gw, bw (endpoint 0) and rx, gx, bx
# (endpoint 1) at bits 5, 15, 25, 35, 45, 55; from bit 65 texel 0's 3-bit index (its top bit is implied 0), then 4 bits for each of texels
# 1 .. 15; texel t = (y & 3) * 4 + (x & 3).  Everything below is integer arithmetic (int64), so every implementation agrees bit for bit.

def _bc6h_weights():
    """The 4-bit interpolation weights W[i] (int64 [16]); W[15 - i] = 64 - W[i]"""
    return np.array((0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64), np.int64)


def lightmap_bc6h_layout(width: int, height: int, levels: int = 0):
    """The block layout of a BC6H mip chain, no GPU needed (render_plan.cpp bc6h_plan is the same rule): [(BW_l, BH_l, offset_l)] for the
    levels of lightmap_mip_layout(width, height, levels): BW_l = (W_l + 3) >> 2 and BH_l likewise blocks of 16 bytes, row-major in the
    level's own row order.  offset_l is where level l starts, in BLOCKS, in the buffer that holds levels 1 .. L - 1 one after the other;
    level 0 is a buffer of its own and its offset is given as 0.  Raises ValueError as lightmap_mip_layout does."""
    out, off = [], 0
    for l, (wl, hl, _) in enumerate(lightmap_mip_layout(width, height, levels)):
        bw, bh = (wl + 3) >> 2, (hl + 3) >> 2
        out.append((bw, bh, off))
        off += bw * bh if l else 0
    return out


def _bc6h_unq(q):
    """A 10-bit endpoint field unquantised to 16 bits (int64 arrays): 0 gives 0, 1023 gives 0xFFFF, every other q gives 64 q + 32"""
    return np.where(q == 0, 0, np.where(q == 1023, 0xFFFF, ((q << 16) + 0x8000) >> 10))


def _bc6h_palette(fields):
    """The sixteen colours a block can hold, as binary16 bits: fields [B, 2, 3] int64 (endpoint, channel) to [B, 16, 3] int64"""
    e = _bc6h_unq(fields)
    w = _bc6h_weights()[None, :, None]
    c = (e[:, 0:1, :] * (64 - w) + e[:, 1:2, :] * w + 32) >> 6
    return (c * 31) >> 6


def _bc6h_quant(c):
    """The 10-bit field whose unquantised value is nearest to c (int64 arrays, clamped to 0 .. 65535 first), the lower field on a tie:
    the three candidates around (c - 1) >> 6 in ascending order, a later one taken only if strictly nearer"""
    c = np.clip(c, 0, 65535)
    q0 = np.clip((c - 1) >> 6, 0, 1023)
    best = np.maximum(q0 - 1, 0)
    bd = np.abs(_bc6h_unq(best) - c)
    for step in (0, 1):
        q = np.minimum(q0 + step, 1023)
        d = np.abs(_bc6h_unq(q) - c)
        take = d < bd
        best, bd = np.where(take, q, best), np.where(take, d, bd)
    return best


def _bc6h_assign(target, fields):
    """Every texel's index by exhaustive search: target [B, 16, 3] binary16 bits, fields [B, 2, 3]; the index whose colour has the least
    squared distance over the three channels, the lowest index on a tie.  Returns (index [B, 16], that distance [B, 16])."""
    d = target[:, :, None, :] - _bc6h_palette(fields)[:, None, :, :]
    e = (d * d).sum(axis=-1)
    idx = e.argmin(axis=-1)                                       # (the first of equal minima)
    return idx, np.take_along_axis(e, idx[..., None], -1)[..., 0]


def _bc6h_blocks_of(plane, bh, bw):
    """[4 bh, 4 bw, ...] as [bh * bw, 16, ...]: texel t = (y & 3) * 4 + (x & 3) of block (y >> 2) * bw + (x >> 2)"""
    tail = plane.shape[2:]
    order = (0, 2, 1, 3) + tuple(range(4, 4 + len(tail)))
    return plane.reshape((bh, 4, bw, 4) + tail).transpose(order).reshape((bh * bw, 16) + tail)


def _bc6h_fit(h, part, rounds):
    """Steps 3 to 6 of lightmap_bc6h_encode for B blocks: h [B, 16, 3] int64 binary16 bits, part [B, 16] bool.  Returns (fields [B, 2, 3],
    index [B, 16]) int64."""
    i64 = np.int64
    n = part.sum(axis=1)
    # 4. the farthest pair
    d = h[:, :, None, :] - h[:, None, :, :]
    d2 = (d * d).sum(axis=-1)
    i, j = np.mgrid[0:16, 0:16]
    both = part[:, :, None] & part[:, None, :] & (i <= j)
    key = np.where(both, d2 * 256 + (255 - (16 * i + j)), -1)
    far = key.reshape(-1, 256).argmax(axis=1)
    at = np.arange(len(h))
    ends = np.stack([h[at, far // 16], h[at, far % 16]], axis=1)
    fields = _bc6h_quant((64 * ends + 30) // 31)
    # 4b. a flat start: a channel whose one field lies more than 32 from its c takes the two fields around c
    c0 = (64 * ends[:, 0] + 30) // 31
    flat = (fields[:, 0] == fields[:, 1]).all(axis=1)
    wide = flat[:, None] & (np.abs(_bc6h_unq(fields[:, 0]) - c0) > 32)
    below = np.where(c0 < 96, 0, 1022)
    fields = np.where(wide[:, None, :], np.stack([below, below + 1], axis=1), fields)
    # 3. the targets and the first indices
    mean = (h * part[..., None]).sum(axis=1) // np.maximum(n, 1)[:, None]
    target = np.where(part[..., None], h, mean[:, None, :])
    idx, e = _bc6h_assign(target, fields)
    err = (e * part).sum(axis=1)
    # 5. least-squares refinement
    w = _bc6h_weights()
    ct = (64 * h + 30) // 31
    for _ in range(rounds):
        u, v = (64 - w[idx]) * part, w[idx] * part
        suu, suv, svv = (u * u).sum(axis=1)[:, None], (u * v).sum(axis=1)[:, None], (v * v).sum(axis=1)[:, None]
        suc, svc = (u[..., None] * ct).sum(axis=1), (v[..., None] * ct).sum(axis=1)
        det = suu * svv - suv * suv
        na, nb = 64 * (svv * suc - suv * svc), 64 * (suu * svc - suv * suc)
        two = 2 * np.maximum(det, 1)
        solved = _bc6h_quant(np.stack([(2 * na + det) // two, (2 * nb + det) // two], axis=1))
        cand = np.where((det != 0)[:, :, None], solved, fields)
        cidx, ce = _bc6h_assign(target, cand)
        cerr = (ce * part).sum(axis=1)
        better = cerr < err
        fields = np.where(better[:, None, None], cand, fields)
        idx, err = np.where(better[:, None], cidx, idx), np.where(better, cerr, err)
    # 6. the anchor, and the blocks in which nothing takes part
    swap = idx[:, 0] >= 8
    fields = np.where(swap[:, None, None], fields[:, ::-1, :], fields)
    idx = np.where(swap[:, None], 15 - idx, idx)
    fields, idx = np.where((n == 0)[:, None, None], 0, fields), np.where((n == 0)[:, None], 0, idx)
    return fields, idx


def check_lightmap_bc6h_image(image, valid=None, rounds: int = 2):
    """Input checking of mi_lightmap_bc6h_encode, no GPU needed: `image` [H, W, 3] with 1 <= W, H <= 32768, `valid` None or [H, W]
    (0 = the texel takes no part), `rounds` 0 .. 4.  Returns (image f32, valid uint8 or None, rounds), contiguous; raises ValueError."""
    img = np.asarray(image, np.float32)
    if img.ndim != 3 or img.shape[2] != 3:
        raise ValueError(f"image must be [H, W, 3], got {np.shape(image)}")
    H, W = img.shape[:2]
    if not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {W} x {H}")
    if not (0 <= int(rounds) <= 4):
        raise ValueError(f"rounds must be in 0 .. 4, got {rounds}")
    v8 = None
    if valid is not None:
        v8 = np.ascontiguousarray(np.asarray(valid) != 0, np.uint8)
        if v8.shape != (H, W):
            raise ValueError(f"valid must be [{H}, {W}], got {v8.shape}")
    return np.ascontiguousarray(img), v8, int(rounds)


def lightmap_bc6h_encode(image, valid=None, rounds: int = 2):
    """Encode an f32 lightmap as BC6H_UF16 blocks on the host (numpy only).  This is the DEFINITION of mi_lightmap_bc6h_encode, which
    equals it byte for byte.  Arguments as check_lightmap_bc6h_image.  Returns uint8 [BH, BW, 16], BH = ceil(H / 4), BW = ceil(W / 4).
    All integer (int64) after step 1.
    1. Per texel and channel: c = min(x, 65504) where x > 0, else 0 (a NaN, a negative, -0.0: 0); h = the round-to-nearest-even binary16
       bits of c, 0 .. 0x7BFF.
    2. A texel TAKES PART when it lies inside the image and valid is None or non-zero there.  One that does not never influences a bit,
       whatever it holds.  A block with no such texel is the word 3 and zeros.
    3. A texel's error is the squared distance of its h to the block's exact decode, summed over channels; a block's error the sum over
       the texels that take part.  Given endpoints every texel has the index of least error, the lowest on a tie; a texel that takes no
       part gets the index that is best for the integer (floor) mean of the h that take part.
    4. Start: the pair (i <= j) of texels that take part farthest apart in h, the lowest (i, j) on a tie; endpoint 0 from texel i,
       endpoint 1 from j.  Per channel c = (64 h + 30) // 31, the smallest c with (c * 31) >> 6 == h, and the field whose unquantised
       value is nearest to c, the lower field on a tie.
    4b. A flat start: if the two endpoints have the same field in every channel, a channel whose field's unquantised value lies more
       than 32 from endpoint 0's c takes the two fields around c instead, (0, 1) where c < 96 and (1022, 1023) otherwise, and the
       indices interpolate.  The unquantised fields are 0, 96, 160, .., 64 q + 32, .., 65440, 65535: only between 0 | 96 and
       65440 | 65535 can the nearest be more than 32 away.  With it a constant block decodes within 16 units of h.
    5. `rounds` times: with u = 64 - W[index], v = W[index] and c as in 4 over the texels that take part, Suu, Suv, Svv, Suc, Svc the sums
       of products and det = Suu Svv - Suv Suv.  Unless det == 0 the endpoints of a channel are a = (2 na + det) // (2 det) with
       na = 64 (Svv Suc - Suv Svc), and b likewise with nb = 64 (Suu Svc - Suv Suc) (floor division: round half up), clamped to
       0 .. 65535 and quantised as in 4.  Indices are assigned again and the result is kept ONLY IF the block's error is strictly lower.
    6. If texel 0's index is 8 or more the endpoints swap and every index i becomes 15 - i (the decode is the same)."""
    img, v8, rounds = check_lightmap_bc6h_image(image, valid, rounds)
    i64 = np.int64
    H, W = img.shape[:2]
    bh, bw = (H + 3) >> 2, (W + 3) >> 2
    with np.errstate(all="ignore"):
        c = np.where(img > 0, np.minimum(img, np.float32(65504.0)), np.float32(0.0))
        bits = c.astype(np.float16).view(np.uint16)
    hp = np.zeros((4 * bh, 4 * bw, 3), i64)
    hp[:H, :W] = bits
    pp = np.zeros((4 * bh, 4 * bw), bool)
    pp[:H, :W] = True if v8 is None else v8 != 0
    h, part = _bc6h_blocks_of(hp, bh, bw), _bc6h_blocks_of(pp, bh, bw)
    fit = [_bc6h_fit(h[k:k + 4096], part[k:k + 4096], rounds) for k in range(0, len(h), 4096)]       # (in chunks: the search is [B, 16, 16, 3])
    fields, idx = np.concatenate([f for f, _ in fit]), np.concatenate([x for _, x in fit])
    f, x = fields.reshape(-1, 6).astype(np.uint64), idx.astype(np.uint64)
    lo = np.full(len(h), 3, np.uint64) | (f[:, 5] & np.uint64(511)) << np.uint64(55)
    for k in range(5):
        lo |= f[:, k] << np.uint64(5 + 10 * k)
    hi = f[:, 5] >> np.uint64(9) | x[:, 0] << np.uint64(1)
    for t in range(1, 16):
        hi |= x[:, t] << np.uint64(4 * t)
    return np.ascontiguousarray(np.stack([lo, hi], axis=1).astype("<u8").view(np.uint8).reshape(bh, bw, 16))


def _check_bc6h_blocks(blocks, width, height):
    """`blocks` as uint8 [BH, BW, 16] for a level of width x height texels (any array of BH * BW * 16 bytes); raises ValueError"""
    W, H = int(width), int(height)
    if not (1 <= W <= 32768 and 1 <= H <= 32768):
        raise ValueError(f"width and height must be in 1 .. 32768, got {W} x {H}")
    b = np.ascontiguousarray(blocks)
    bw, bh = (W + 3) >> 2, (H + 3) >> 2
    if b.dtype != np.uint8 or b.size != bh * bw * 16:
        raise ValueError(f"blocks must be uint8 [{bh}, {bw}, 16] for {W} x {H} texels, got {b.dtype} {b.shape}")
    return b.reshape(bh, bw, 16)


def lightmap_bc6h_modes(blocks):
    """The histogram of the low five bits of BC6H blocks (uint8 [..., 16]): int64 [32].  lightmap_bc6h_decode and the kernels read the
    blocks counted at [3] and give zeros for all others, so a file is readable here when every block is counted there."""
    b = np.ascontiguousarray(blocks)
    if b.dtype != np.uint8 or b.ndim < 1 or b.shape[-1] != 16:
        raise ValueError(f"blocks must be uint8 [..., 16], got {b.dtype} {b.shape}")
    return np.bincount((b[..., 0] & 31).reshape(-1), minlength=32).astype(np.int64)


def lightmap_bc6h_decode(blocks, width: int, height: int):
    """Decode BC6H_UF16 blocks on the host (numpy only).  This is the DEFINITION of mi_lightmap_bc6h_decode: uint8 [BH, BW, 16] to f32
    [height, width, 3].  A block whose low five bits are not 3 (every two-region, delta or reserved mode) decodes to zeros.  Otherwise,
    with a, b the unquantised fields of a channel (0 gives 0, 1023 gives 0xFFFF, else ((q << 16) + 0x8000) >> 10) and i the texel's index:
    c = (a (64 - W[i]) + b W[i] + 32) >> 6, h = (c * 31) >> 6, and h read as binary16 bits, widened exactly to f32 (h <= 0x7BFF)."""
    b = _check_bc6h_blocks(blocks, width, height)
    bh, bw = b.shape[:2]
    words = b.reshape(-1, 16).view("<u8").astype(np.uint64)
    lo, hi = words[:, 0], words[:, 1]
    f = [(lo >> np.uint64(5 + 10 * k)) & np.uint64(1023) for k in range(5)] + [(lo >> np.uint64(55) | hi << np.uint64(9)) & np.uint64(1023)]
    fields = np.stack(f, axis=1).astype(np.int64).reshape(-1, 2, 3)
    idx = np.stack([(hi >> np.uint64(1)) & np.uint64(7)] + [(hi >> np.uint64(4 * t)) & np.uint64(15) for t in range(1, 16)], axis=1).astype(np.int64)
    h = np.take_along_axis(_bc6h_palette(fields), idx[:, :, None], axis=1)
    h = np.where(((lo & np.uint64(31)) == 3)[:, None, None], h, 0)
    texels = h.reshape(bh, bw, 4, 4, 3).transpose(0, 2, 1, 3, 4).reshape(4 * bh, 4 * bw, 3)[:int(height), :int(width)]
    return np.ascontiguousarray(texels.astype(np.uint16).view(np.float16).astype(np.float32))


def lightmap_bc6h_chain(chain, valid_chain=None, rounds: int = 2):
    """Encode every level of a lightmap_mips chain ([H_l, W_l, 3] f32, level 0 first) with its own mask (valid_chain None: everything takes
    part; lightmap_mips' second list otherwise; an entry may be None).  Returns the list of uint8 [BH_l, BW_l, 16]."""
    chain = list(chain) if isinstance(chain, (list, tuple)) else [chain]
    masks = [None] * len(chain) if valid_chain is None else list(valid_chain)
    if len(masks) != len(chain):
        raise ValueError(f"valid_chain must be None or a list of {len(chain)} masks")
    return [lightmap_bc6h_encode(a, m, rounds) for a, m in zip(chain, masks)]


def check_lightmap_bc6h(blocks_chain, width: int, height: int, uv, lod=None, valid_chain=None, flags: int = 0):
    """Input checking of mi_lightmap_sample_bc6h, no GPU needed.  `blocks_chain` is a list of block arrays as lightmap_bc6h_chain returns
    them, level 0 first (sizes: lightmap_bc6h_layout(width, height, L)), or one array.  The rest is checked on the decoded levels as
    check_lightmap_lod checks it, or with lod None as check_lightmap_lookup does (abi.MI_LS_NEAREST allowed; one level alone).  Returns
    (blocks [L] contiguous uint8 [BH_l, BW_l, 16], what the f32 check returned for the decoded levels); raises ValueError."""
    chain = list(blocks_chain) if isinstance(blocks_chain, (list, tuple)) else [blocks_chain]
    if len(chain) == 0:
        raise ValueError("blocks_chain must hold level 0")
    layout = lightmap_mip_layout(width, height, len(chain))
    blocks = [_check_bc6h_blocks(b, wl, hl) for b, (wl, hl, _) in zip(chain, layout)]
    levels = [lightmap_bc6h_decode(b, wl, hl) for b, (wl, hl, _) in zip(blocks, layout)]
    return blocks, _check_level_form(levels, uv, lod, valid_chain, flags)


def lightmap_sample_bc6h(blocks_chain, width: int, height: int, uv, lod=None, valid_chain=None, flags: int = 0):
    """Read a BC6H lightmap at uv points on the host (numpy only).  This is the DEFINITION of mi_lightmap_sample_bc6h: decode every
    level, then lightmap_sample_lod — or, with lod None, lightmap_sample of the one level (bilinear or abi.MI_LS_NEAREST).  Arguments as
    check_lightmap_bc6h.  Returns (out [..., 3] f32, weight [...] f32)."""
    return _sample_level_form(check_lightmap_bc6h(blocks_chain, width, height, uv, lod, valid_chain, flags)[1], lod)


class Bc6hLightmap:
    """A plain (irradiance) lightmap stored as BC6H blocks, for Scene.shade_rays_baked and shade_hits_baked: `blocks_chain` as
    lightmap_bc6h_chain returns it for a lightmap of width x height texels, `valid_chain` its masks or None, `lod` None (level 0 alone:
    then the chain is one level) or the lod every hit is read at."""

    def __init__(self, blocks_chain, width: int, height: int, valid_chain=None, lod=None):
        self.blocks_chain = list(blocks_chain) if isinstance(blocks_chain, (list, tuple)) else [blocks_chain]
        self.width, self.height, self.valid_chain, self.lod = int(width), int(height), valid_chain, lod


def lightmap_finish_var(image, m2, samples, points, normals, levels: int = 3, normal_power_log2: int = 5,
                        sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = 8.0,
                        color_floor: float = 1e-6, dilate: int = 4):
    """lightmap_finish with a variance-guided colour weight (numpy only).  This is the DEFINITION of mi_lightmap_finish_var, which equals
    it bit for bit.  `image` and `m2` [H, W, 3] f32 are the mean and the mean of squares of a bake of `samples` = S samples per texel
    (bake_lightmap_moments), `points` and `normals` the centre table, as for lightmap_finish.  Returns (out [H, W, 3] f32,
    var [H, W] f32, valid [H, W] bool).  The coverage rule, the tap order, h, wn, wp, the reach test, the centre tap's exemption and the
    dilation are lightmap_finish's; everything is f32, one rounding per operation, in the order of the building blocks above.
    Initial variance of the mean, covered texels: v_c = max(0, m2_c - mean_c mean_c) / (S - 1), V = (v_r + v_g) + v_b; empty texels +0.0.
    The difference cancels in f32: V means nothing where the true noise is below about 1e-3 of the mean; `color_floor` is for that case.
    Per level (step s = 2^i): first the blur, bs = sum g V_q and bw = sum g over the nine neighbours at step 1 (whatever s is) that lie
    in the image and are covered, g = G3[dy] G3[dx], G3 = (1/4, 1/2, 1/4); sd = sqrt(bs / bw), den = sigma_color sd + color_floor.  Then
    the a-trous level with the colour weight max(0, 1 - (|dr| + |dg| + |db|) / den), den taken at p only and not divided by s, and
    beside sw and sc the sum sv = sv + (w w) V_q: the texel becomes sc / sw, its variance sv / (sw sw).  color_floor = inf turns the
    colour weight off: the image is then lightmap_finish(sigma_color=inf)'s, bit for bit.
    `var` is the final V for covered texels and +0.0 elsewhere, dilated texels included; levels == 0 gives the masked copy and the
    initial V.  Non-finite values spoil the texels within Chebyshev radius 2 (2^levels - 1) + levels + dilate, and no others.
    `samples` may also be an [H, W] integer array, the per-texel counts of an adaptive bake (the definition of
    mi_lightmap_finish_var_counts): the initial variance then divides by the texel's own n - 1, and a texel with n < 2 starts from
    V = +0.0.  A plane that holds one value S everywhere gives the result of samples = S, bit for bit."""
    f32 = np.float32
    img, P, N = check_finish_tables(image, points, normals)
    M2 = np.ascontiguousarray(m2, f32)
    if M2.shape != img.shape:
        raise ValueError(f"m2 must have the image's shape {img.shape}, got {M2.shape}")
    if np.ndim(samples) != 0:                # a plane of per-texel counts (mi_lightmap_finish_var_counts)
        n = check_counts_plane(samples, img.shape[:2])
    else:
        n = int(samples)
        if not 2 <= n <= 65535:
            raise ValueError(f"samples must be in 2 .. 65535, got {samples}")
    levels, npow, dilate = _check_finish_passes(levels, normal_power_log2, dilate)
    sig_p, rch, sig_c0, floor = f32(sigma_plane), f32(reach), f32(sigma_color), f32(color_floor)
    if not (sig_p > 0 and rch > 0):
        raise ValueError("sigma_plane and reach must be > 0 (inf turns one off)")
    if not (sig_c0 >= 0 and np.isfinite(sig_c0)):
        raise ValueError("sigma_color must be finite and >= 0")
    if not floor > 0:
        raise ValueError("color_floor must be > 0 (inf turns the colour weight off)")
    covered = _lm_covered(N)
    cur = np.where(covered[..., None], img, f32(0.0))
    with np.errstate(all="ignore"):
        V = _lmv_variance(cur, M2, n, covered, f32(0.0))
        for level in range(levels):
            s = 1 << level
            bs, bw = _lmv_blur(V, N, covered, 1)              # always at step 1, whatever s is
            sd = np.sqrt(bs / bw)
            den = sig_c0 * sd + floor
            cur, V = _lmf_level(cur, P, N, covered, s, npow, sig_p, rch, den, V)
        cur, valid = _lmf_dilate(cur, covered, dilate)
    return cur, np.ascontiguousarray(V, f32), valid


def check_counts_plane(counts, shape):
    """An [H, W] array of per-texel sample counts as contiguous uint32: an integer dtype, the given shape, values in 0 .. 2^32 - 1"""
    c = np.asarray(counts)
    if c.dtype.kind not in "iu":
        raise ValueError(f"counts must be an integer array, got {c.dtype}")
    if c.shape != tuple(shape):
        raise ValueError(f"counts must have shape {tuple(shape)}, got {c.shape}")
    if c.size and (int(c.min()) < 0 or int(c.max()) > 0xffffffff):
        raise ValueError("counts must lie in 0 .. 2^32 - 1")
    return np.ascontiguousarray(c, np.uint32)


def _check_index_list(index):
    idx = np.asarray(index)
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise ValueError(f"index must be a 1-d integer array, got {idx.dtype} {idx.shape}")
    if idx.size and (int(idx.min()) < 0 or int(idx.max()) > 0xffffffff):
        raise ValueError("index entries must lie in 0 .. 2^32 - 1")
    return np.ascontiguousarray(idx, np.uint32)


def lightmap_select(image, m2, counts, normals, target_rel: float, target_abs: float, capacity: Optional[int] = None):
    """The texels of a bake that are worth further samples (numpy only).  This is the DEFINITION of mi_lightmap_select, which equals it
    bit for bit.  `image` and `m2` [H, W, 3] f32 are the bake's running mean and mean of squares, `counts` [H, W] integers the samples
    behind each texel, `normals` [H, W, 3] the centre table (an all-zero normal: an empty texel, never selected).
    Per covered texel with n = counts: n >= 2 gives v_c = max(0, m2_c - mean_c mean_c) / (n - 1), V = (v_r + v_g) + v_b, the variance of
    the mean (lightmap_finish_var's initial variance with the texel's own n); n < 2 gives V = +inf: no information, always selected.
    Empty texels +0.0.  Then sd = sqrt(bs / bw) with lightmap_finish_var's blur (the nine step-1 neighbours that lie in the image and are
    covered, dy outer, dx inner, g = G3[dy] G3[dx]): a dark texel whose few samples all missed the light is judged with its neighbours.
    With lum = (|mean_r| + |mean_g|) + |mean_b| the texel is selected when sd > target_rel * lum + target_abs.  Everything is f32, one
    rounding per operation.  Returns (index, count, error): the selected texel numbers y * W + x ascending as uint32, the lowest
    `capacity` of them (None: all); count, the number of selected texels whatever the capacity; error [H, W] f32, sd (+0.0 on empty
    texels).  A non-finite texel changes the selection within Chebyshev distance 1 only."""
    f32 = np.float32
    img, M2, N = check_finish_tables(image, m2, normals)
    cnt = check_counts_plane(counts, img.shape[:2])
    trel, tabs = f32(target_rel), f32(target_abs)
    if not (trel >= 0 and tabs >= 0):
        raise ValueError("target_rel and target_abs must be >= 0 and not NaN")
    H, W = img.shape[:2]
    cap = H * W if capacity is None else int(capacity)
    if not 0 <= cap <= 0xffffffff:
        raise ValueError(f"capacity must be in 0 .. 2^32 - 1, got {capacity}")
    zero = f32(0.0)
    covered = _lm_covered(N)
    with np.errstate(all="ignore"):
        V = _lmv_variance(img, M2, cnt, covered, f32(np.inf))
        bs, bw = _lmv_blur(V, N, covered, 1)
        sd = np.where(covered, np.sqrt(bs / bw), zero).astype(f32)
        lum = (np.abs(img[..., 0]) + np.abs(img[..., 1])) + np.abs(img[..., 2])
        thr = trel * lum + tabs
        selected = covered & (sd > thr)
    index = np.flatnonzero(selected).astype(np.uint32)
    return index[:cap], int(index.size), np.ascontiguousarray(sd, f32)


def lightmap_gather(index, points, normals, cw: int):
    """The compact point table of a list of texels (numpy only): the DEFINITION of mi_lightmap_gather.  `index` holds n texel numbers
    y * W + x, `points` and `normals` are [rows, H, W, 3] (or [H, W, 3]) f32.  Returns (points, normals) [rows, ch, cw, 3] with
    ch = ceil(n / cw): entry i goes to slot (i // cw, i % cw) of every row; the slots at or after n are all zero, the empty-texel mark
    (render_points traces nothing for them), and so is the slot of an index >= W * H."""
    idx = _check_index_list(index)
    P, N = np.asarray(points), np.asarray(normals)
    if P.dtype != np.float32 or N.dtype != np.float32:
        raise ValueError(f"points and normals must be float32, got {P.dtype} and {N.dtype}")
    if P.ndim == 3:
        P = P[None]
    if N.ndim == 3:
        N = N[None]
    if P.ndim != 4 or P.shape[3] != 3 or P.shape != N.shape:
        raise ValueError(f"points and normals must be [rows, H, W, 3] arrays of one shape, got {P.shape} and {N.shape}")
    rows, H, W = P.shape[:3]
    if not (1 <= W <= 32768 and 1 <= H <= 32768 and 1 <= rows <= 65535):
        raise ValueError(f"width and height must be in 1 .. 32768 and rows in 1 .. 65535, got {W} x {H} x {rows}")
    cw, n = int(cw), int(idx.size)
    if not 1 <= cw <= 32768:
        raise ValueError(f"cw must be in 1 .. 32768, got {cw}")
    ch = (n + cw - 1) // cw
    if not 1 <= ch <= 32768:
        raise ValueError(f"{n} entries at cw = {cw} give {ch} rows of slots: not in 1 .. 32768")
    ok = idx < W * H
    outs = []
    for t in (P, N):
        out = np.zeros((rows, ch * cw, 3), np.float32)
        out[:, np.flatnonzero(ok)] = t.reshape(rows, H * W, 3)[:, idx[ok]]
        outs.append(out.reshape(rows, ch, cw, 3))
    return outs[0], outs[1]


def lightmap_merge(index, mean, m2_round, round_samples: int, image, m2, counts):
    """Merge a refinement round into a bake (numpy only): the DEFINITION of mi_lightmap_merge.  `index` lists n texels; `mean` and
    `m2_round` hold, in their first n slots ([ch, cw, 3], or any shape of at least n triples), the mean and mean of squares of a round of
    `round_samples` = S' samples of those texels; `image`, `m2` [H, W, 3] f32 and `counts` [H, W] are the bake so far.  For each listed
    texel with count n0, per channel: image = (n0 * image + S' * mean') / (n0 + S') in f32, one rounding per operation, m2 likewise,
    counts = n0 + S'.  Every other texel keeps its bits; an index >= W * H is skipped.  Returns new (image, m2, counts uint32).  A list
    with duplicates is refused (the kernel runs one lane per entry)."""
    f32 = np.float32
    idx = _check_index_list(index)
    img, M2, _ = check_finish_tables(image, m2, m2)
    cnt = check_counts_plane(counts, img.shape[:2]).copy()
    S = int(round_samples)
    if not 1 <= S <= 65535:
        raise ValueError(f"round_samples must be in 1 .. 65535, got {round_samples}")
    n = int(idx.size)
    mr, m2r = np.ascontiguousarray(mean, f32).reshape(-1), np.ascontiguousarray(m2_round, f32).reshape(-1)
    if mr.size < 3 * n or m2r.size < 3 * n or mr.size % 3 or m2r.size % 3:
        raise ValueError(f"mean and m2_round must hold at least {n} triples, got {mr.size} and {m2r.size} values")
    H, W = img.shape[:2]
    ok = idx < W * H
    t = idx[ok].astype(np.int64)
    if np.unique(t).size != t.size:
        raise ValueError("index lists a texel twice")
    img, M2 = img.copy().reshape(-1, 3), M2.copy().reshape(-1, 3)
    n0_int = cnt.reshape(-1)[t].astype(np.int64)
    n0, Sf, tot = n0_int.astype(f32)[:, None], f32(S), (n0_int + S).astype(f32)[:, None]
    with np.errstate(all="ignore"):
        for plane, new in ((img, mr), (M2, m2r)):
            a, b = plane[t], new.reshape(-1, 3)[:n][ok]
            plane[t] = (n0 * a + Sf * b) / tot
    cnt.reshape(-1)[t] = ((n0_int + S) & 0xffffffff).astype(np.uint32)
    return img.reshape(H, W, 3), M2.reshape(H, W, 3), cnt


def equirect_dirs(lon, lat) -> np.ndarray:
    """Unit directions [..., 3] float32 of a latitude-longitude panorama for arrays of longitudes / latitudes in radians:
    (sin lon cos lat, sin lat, -cos lon cos lat) — longitude 0 looks down -z, +pi/2 down +x, +-pi (the seam) down +z; latitude +pi/2 is
    +y.  Multiples of pi/2 go through exact sines and cosines, so the poles, the seam and +-x / -z are axis-aligned to the last bit."""
    lon, lat = np.broadcast_arrays(np.asarray(lon, np.float64), np.asarray(lat, np.float64))

    def exact(table, f, a):
        q = a / (0.5 * np.pi)
        r = np.rint(q)
        return np.where(np.abs(q - r) < 1e-12, np.take(np.array(table), r.astype(np.int64) % 4), f(a))
    sl, cl = exact((0.0, 1.0, 0.0, -1.0), np.sin, lon), exact((1.0, 0.0, -1.0, 0.0), np.cos, lon)
    sp, cp = exact((0.0, 1.0, 0.0, -1.0), np.sin, lat), exact((1.0, 0.0, -1.0, 0.0), np.cos, lat)
    d = np.stack([sl * cp, sp, -cl * cp], axis=-1) + 0.0              # + 0.0: no negative zeros
    return np.ascontiguousarray(d, dtype=np.float32)


def equirect_ray_table(width: int, height: int, eye, samples: int = 1, seed: int = 0):
    """A latitude-longitude panorama seen from `eye` as a ray table for render_rays: (origins, dirs), each [samples, height, width, 3]
    float32, unit directions (equirect_dirs).  Columns span the longitudes [-pi, pi) from left to right, rows the latitudes from +pi/2
    at the top edge to -pi/2 at the bottom edge.  Sample s of pixel (x, y) looks through the image point (x + jx, y + jy): the pixel
    centre for samples == 1, otherwise a jitter in [0, 1)^2 drawn from numpy's default_rng(seed) — the same seed gives the same table."""
    W, H, S = int(width), int(height), int(samples)
    if W < 1 or H < 1 or S < 1:
        raise ValueError("width, height and samples must be >= 1")
    if S == 1:
        jx = jy = np.full((1, H, W), 0.5)
    else:
        j = np.random.default_rng(seed).random((2, S, H, W))
        jx, jy = j[0], j[1]
    lon = ((np.arange(W)[None, None, :] + jx) / W - 0.5) * (2.0 * np.pi)
    lat = (0.5 - (np.arange(H)[None, :, None] + jy) / H) * np.pi
    dirs = equirect_dirs(lon, lat)
    origins = np.ascontiguousarray(np.broadcast_to(np.asarray(eye, np.float32).reshape(3), dirs.shape))
    return origins, dirs


def mesh_pod(mesh, transform=None):
    """(abi.mi_mesh, what keeps its arrays alive) for mi_lightmap_texels / mi_bake_lightmap: `mesh` is a StaticMesh (geometry.py; its
    own transform unless one is given) or an objload.Mesh (identity unless one is given).  Only the four arrays, the two counts and the
    transform are filled in: the calls read nothing else."""
    from . import cgmath
    if hasattr(mesh, "mesh") and hasattr(mesh, "transform"):              # a StaticMesh
        transform = mesh.transform if transform is None else transform
        mesh = mesh.mesh
    M = np.asarray(cgmath.identity() if transform is None else transform, np.float32).reshape(4, 4)
    keep = [np.ascontiguousarray(mesh.positions, np.float32).reshape(-1), np.ascontiguousarray(mesh.normals, np.float32).reshape(-1),
            np.ascontiguousarray(mesh.texcoords, np.float32).reshape(-1), np.ascontiguousarray(mesh.indices, np.uint32).reshape(-1)]
    if keep[1].size != keep[0].size or keep[2].size * 3 != keep[0].size * 2 or keep[0].size % 3 or keep[3].size % 3:
        raise ValueError("mesh needs positions and normals [V, 3], texcoords [V, 2] and indices [T, 3]")
    pod = abi.mi_mesh()
    pod.positions, pod.normals, pod.texcoords = (a.ctypes.data_as(C.POINTER(C.c_float)) for a in keep[:3])
    pod.indices = keep[3].ctypes.data_as(C.POINTER(C.c_uint32))
    pod.n_vertices, pod.n_triangles = keep[0].size // 3, keep[3].size // 3
    pod.transform = abi.f16(*cgmath.cols16(M))
    pod.material = -1
    return pod, keep


class Context:
    """One mi_ctx = one GPU (one process per GPU: pass LOCAL_RANK)."""

    def __init__(self, device: int = 0, _borrowed=None):
        self._lib = abi.load()
        self._h = C.c_void_p()
        self._owned = _borrowed is None
        if _borrowed is None:
            abi.check(self._lib.mi_ctx_create(device, C.byref(self._h)))
        else:                                  # a device context owned by a MultiContext (mi_multi_context)
            self._h = C.c_void_p(_borrowed)
        self.device = device

    def close(self):
        if self._h and self._owned:
            self._lib.mi_ctx_destroy(self._h)
        self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, flat: FlatScene):
        abi.check(self._lib.mi_scene_upload(self._h, C.byref(flat.desc)))

    def render(self, cam: Camera, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
               variant: int = abi.MI_VARIANT_DEFAULT, flags: int = 0, max_state_bytes: int = 0):
        """mi_render: whole image on this GPU.  Returns (f32 [H,W,3] | None, u8 [H,W,3] | None,
        sig [H,W] | None, mi_stats)."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=variant, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_render(
            self._h, C.byref(pod), C.byref(opts),
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None, C.byref(st)))
        return f32, u8, sig, st

    def render_rays(self, cam: Camera, origins, dirs, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
                    flags: int = 0, max_state_bytes: int = 0):
        """mi_render_rays: the whole image from a ray table (check_ray_table: [S, H, W, 3] or [H, W, 3] float32, S = 1 or
        aa_sample_count) instead of Camera::generate_rays, through the wavefront pipeline.  Sample s of pixel (x, y) draws from the stream
        (seed, y*W + x, s).  Returns what render returns."""
        o, d, rows = check_ray_table(cam, origins, dirs)
        return self._render_table(self._lib.mi_render_rays, cam, o, d, rows, seed, want_f32, want_u8, want_sig, flags, max_state_bytes)

    def _render_table(self, entry, cam, first, second, rows, seed, want_f32, want_u8, want_sig, flags, max_state_bytes):
        """mi_render_rays / mi_render_points on checked, contiguous host tables"""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        st = abi.mi_stats()
        abi.check(entry(
            self._h, C.byref(pod), C.byref(opts), first.ctypes.data, second.ctypes.data, rows,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None, C.byref(st)))
        return f32, u8, sig, st

    def render_points(self, cam: Camera, points, normals, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
                      flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points: the whole image from a point table (check_point_table: surface points and normals, [S, H, W, 3] or
        [H, W, 3] float32, S = 1 or aa_sample_count), the directions drawn on the GPU: sample s of pixel (x, y) leaves its point along
        sample_hemisphere(normal) from the stream (seed, W*H + y*W + x, s) and its path draws from (seed, y*W + x, s).  A zero normal is
        an empty texel (black).  Returns what render returns."""
        p, n, rows = check_point_table(cam, points, normals)
        return self._render_table(self._lib.mi_render_points, cam, p, n, rows, seed, want_f32, want_u8, want_sig, flags, max_state_bytes)

    def lightmap_texels(self, mesh, width: int, height: int, rows: int = 1, jitter: bool = False, seed: int = 1, offset: float = 0.0,
                        transform=None, want_triangle: bool = True):
        """mi_lightmap_texels: the point table of a mesh's uv atlas, made on the GPU — what the helper lightmap_texels computes on the
        host, sample by sample.  `mesh` is a StaticMesh (its transform is used unless `transform` is given) or an objload.Mesh.  Returns
        (points [rows, H, W, 3] f32, normals [rows, H, W, 3] f32, triangle [rows, H, W] int32 | None): the winning triangle per sample,
        -1 and a zero normal where the texel is empty.  With jitter, row r of texel (x, y) sits at lightmap_jitter(...)[r, y, x];
        without, every row is the texel's centre.  No scene is needed."""
        pod, keep = mesh_pod(mesh, transform)
        shape = (max(int(rows), 0), max(int(height), 0), max(int(width), 0))
        pts = np.empty(shape + (3,), np.float32)
        nrm = np.empty(shape + (3,), np.float32)
        tri = np.empty(shape, np.int32) if want_triangle else None
        abi.check(self._lib.mi_lightmap_texels(self._h, C.byref(pod), width, height, rows, abi.MI_LM_JITTER if jitter else 0, seed, offset,
                                               pts.ctypes.data, nrm.ctypes.data, tri.ctypes.data if tri is not None else None))
        del keep
        return pts, nrm, tri

    def lightmap_texels_device(self, d_positions: int, d_normals: int, d_texcoords: int, d_indices: int, n_vertices: int, n_triangles: int,
                               width: int, height: int, d_out_points: int, d_out_normals: int, d_out_triangle: Optional[int] = None,
                               rows: int = 1, jitter: bool = False, seed: int = 1, offset: float = 0.0, transform=None,
                               stream: Optional[int] = None):
        """mi_lightmap_texels_device: the same for a mesh and tables held on the device (raw pointers, e.g. tensor.data_ptr(): positions
        and normals [V, 3] f32, texcoords [V, 2] f32, indices [T, 3] u32; outputs [rows, H, W, 3] f32 and [rows, H, W] int32).  Queued on
        `stream`; the tables can go straight into render_points_device.  A triangle with an index >= n_vertices covers nothing."""
        pod = abi.mi_mesh()
        pod.positions = C.cast(d_positions, C.POINTER(C.c_float))
        pod.normals = C.cast(d_normals, C.POINTER(C.c_float))
        pod.texcoords = C.cast(d_texcoords, C.POINTER(C.c_float))
        pod.indices = C.cast(d_indices, C.POINTER(C.c_uint32))
        pod.n_vertices, pod.n_triangles = n_vertices, n_triangles
        from . import cgmath
        pod.transform = abi.f16(*cgmath.cols16(np.asarray(cgmath.identity() if transform is None else transform, np.float32).reshape(4, 4)))
        abi.check(self._lib.mi_lightmap_texels_device(self._h, C.byref(pod), width, height, rows, abi.MI_LM_JITTER if jitter else 0, seed,
                                                      offset, d_out_points, d_out_normals, d_out_triangle, stream))

    def bake_lightmap(self, cam: Camera, mesh, jitter: bool = True, offset: float = 1e-3, seed: int = 1, transform=None, want_f32=True,
                      want_u8=True, want_sig=False, want_triangle=False, flags: int = 0, max_state_bytes: int = 0):
        """mi_bake_lightmap: lightmap_texels and render_points in one call, the table never leaving the GPU.  The atlas is
        cam.screen_width x screen_height; with jitter every one of the aa_sample_count samples of a texel starts at its own position
        inside the texel.  Returns (f32, u8, sig, triangle [rows, H, W] int32 | None, stats)."""
        pod, keep = mesh_pod(mesh, transform)
        cpod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        tri = np.empty((cam.aa_sample_count if jitter else 1, H, W), np.int32) if want_triangle else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_bake_lightmap(
            self._h, C.byref(cpod), C.byref(opts), C.byref(pod), abi.MI_LM_JITTER if jitter else 0, offset,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None,
            tri.ctypes.data if tri is not None else None, C.byref(st)))
        del keep
        return f32, u8, sig, tri, st

    def lightmap_finish(self, image, points, normals, levels: int = 3, normal_power_log2: int = 5, sigma_plane: float = float("inf"),
                        reach: float = float("inf"), sigma_color: float = float("inf"), dilate: int = 4):
        """mi_lightmap_finish: the edge-aware a-trous filter and the gutter dilation of the helper lightmap_finish on the GPU, bit for
        bit.  `image` is the raw bake [H, W, 3] f32, `points` and `normals` the atlas's centre table ([H, W, 3], or lightmap_texels'
        [1, H, W, 3]).  Returns (out [H, W, 3] f32, valid [H, W] bool).  No scene is needed."""
        img, P, N = check_finish_tables(image, _centre_table(points), _centre_table(normals))
        H, W = img.shape[:2]
        out = np.empty((H, W, 3), np.float32)
        valid = np.empty((H, W), np.uint8)
        abi.check(self._lib.mi_lightmap_finish(self._h, W, H, img.ctypes.data, P.ctypes.data, N.ctypes.data, levels, normal_power_log2,
                                               sigma_plane, reach, sigma_color, dilate, out.ctypes.data, valid.ctypes.data))
        return out, valid.astype(bool)

    def lightmap_finish_device(self, width: int, height: int, d_image: int, d_points: int, d_normals: int, d_out_image: int,
                               d_out_valid: Optional[int] = None, levels: int = 3, normal_power_log2: int = 5,
                               sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = float("inf"),
                               dilate: int = 4, stream: Optional[int] = None):
        """mi_lightmap_finish_device: the same for an image and a table held on the device (raw pointers, e.g. tensor.data_ptr(): three
        [H, W, 3] f32 inputs, the [H, W, 3] f32 output, which must overlap none of them, and an optional [H, W] u8 mask).  Queued on
        `stream`; the output can go straight into tonemap_device."""
        abi.check(self._lib.mi_lightmap_finish_device(self._h, width, height, d_image, d_points, d_normals, levels, normal_power_log2,
                                                      sigma_plane, reach, sigma_color, dilate, d_out_image, d_out_valid, stream))

    # ---- directional lightmaps: the SH L2 records of a bake, their finish and their evaluation ----
    def _render_sh(self, entry, cam, head, want_f32, want_u8, want_sig, tri_rows, seed, flags, max_state_bytes):
        """mi_render_points_sh / mi_bake_lightmap_sh: `head` holds the arguments between opts and out_sh"""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        sh = np.empty((H, W, 9, 3), np.float32)
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        tri = np.empty((tri_rows, H, W), np.int32) if tri_rows else None
        st = abi.mi_stats()
        outs = [f32.ctypes.data if f32 is not None else None, u8.ctypes.data if u8 is not None else None,
                sig.ctypes.data if sig is not None else None]
        if tri_rows is not None:
            outs.append(tri.ctypes.data if tri is not None else None)
        abi.check(entry(self._h, C.byref(pod), C.byref(opts), *head, sh.ctypes.data, *outs, C.byref(st)))
        return sh, f32, u8, sig, tri, st

    def render_points_sh(self, cam: Camera, points, normals, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
                         flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points_sh: render_points with the per-texel SH L2 radiance records as a further output.  Returns
        (sh [H, W, 9, 3] f32, f32, u8, sig, stats): sh[k] = (2 pi / S) sum_s L_s Y_k(d_s / |d_s|) over the texel's hemisphere
        directions, each sum an f32 chain in sample order (lightmap_sh_eval turns it into irradiance at any normal); the rest is what
        render_points returns, bit for bit."""
        p, n, rows = check_point_table(cam, points, normals)
        sh, f32, u8, sig, _, st = self._render_sh(self._lib.mi_render_points_sh, cam, (p.ctypes.data, n.ctypes.data, rows), want_f32,
                                                  want_u8, want_sig, None, seed, flags, max_state_bytes)
        return sh, f32, u8, sig, st

    def render_points_sh_device(self, cam: Camera, d_points: int, d_normals: int, rows_per_pixel: int,
                                d_compact_sh: Optional[int] = None, d_compact: Optional[int] = None, d_sig: Optional[int] = None,
                                sample_begin: int = 0, sample_end: Optional[int] = None, d_accum: Optional[int] = None, seed: int = 1,
                                rank: int = 0, world: int = 1, stream: Optional[int] = None, flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points_sh_device: render_points_device with d_compact_sh, [compact_size(...)[1] * 1024, 9, 3] float32 in the
        compact layout, the SH output and its running accumulator across progressive calls with render_probes_device's rules
        (started by the call with sample_begin == 0, scaled by the one that reaches aa_sample_count); None is exactly
        render_points_device."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=abi.MI_VARIANT_DEFAULT,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        end = cam.aa_sample_count if sample_end is None else sample_end
        abi.check(self._lib.mi_render_points_sh_device(self._h, C.byref(pod), C.byref(opts), d_points, d_normals, rows_per_pixel,
                                                       sample_begin, end, d_accum, d_compact_sh, d_compact, d_sig, stream, C.byref(st)))
        return st

    def bake_lightmap_sh(self, cam: Camera, mesh, jitter: bool = True, offset: float = 1e-3, seed: int = 1, transform=None,
                         want_f32=True, want_u8=True, want_sig=False, want_triangle=False, flags: int = 0, max_state_bytes: int = 0):
        """mi_bake_lightmap_sh: bake_lightmap with the SH L2 records.  Returns (sh [H, W, 9, 3] f32, f32, u8, sig, triangle, stats);
        everything behind sh is what bake_lightmap returns, bit for bit."""
        pod, keep = mesh_pod(mesh, transform)
        out = self._render_sh(self._lib.mi_bake_lightmap_sh, cam, (C.byref(pod), abi.MI_LM_JITTER if jitter else 0, offset), want_f32,
                              want_u8, want_sig, (cam.aa_sample_count if jitter else 1) if want_triangle else 0, seed, flags,
                              max_state_bytes)
        del keep
        return out

    def lightmap_finish_sh(self, sh, points, normals, levels: int = 3, normal_power_log2: int = 5, sigma_plane: float = float("inf"),
                           reach: float = float("inf"), sigma_color: float = float("inf"), dilate: int = 4):
        """mi_lightmap_finish_sh: the helper lightmap_finish_sh on the GPU, bit for bit.  `sh` is the raw bake [H, W, 9, 3] f32,
        `points` and `normals` the atlas's centre table ([H, W, 3], or lightmap_texels' [1, H, W, 3]).  Returns
        (out [H, W, 9, 3] f32, valid [H, W] bool).  No scene is needed."""
        S, P, N = check_finish_sh_tables(sh, points, normals)
        H, W = S.shape[:2]
        out = np.empty((H, W, 9, 3), np.float32)
        valid = np.empty((H, W), np.uint8)
        abi.check(self._lib.mi_lightmap_finish_sh(self._h, W, H, S.ctypes.data, P.ctypes.data, N.ctypes.data, levels, normal_power_log2,
                                                  sigma_plane, reach, sigma_color, dilate, out.ctypes.data, valid.ctypes.data))
        return out, valid.astype(bool)

    def lightmap_finish_sh_device(self, width: int, height: int, d_sh: int, d_points: int, d_normals: int, d_out_sh: int,
                                  d_out_valid: Optional[int] = None, levels: int = 3, normal_power_log2: int = 5,
                                  sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = float("inf"),
                                  dilate: int = 4, stream: Optional[int] = None):
        """mi_lightmap_finish_sh_device: the same for records and a table held on the device (raw pointers: [H, W, 9, 3] f32 in and
        out, which must not overlap, two [H, W, 3] f32 guides and an optional [H, W] u8 mask).  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_finish_sh_device(self._h, width, height, d_sh, d_points, d_normals, levels, normal_power_log2,
                                                         sigma_plane, reach, sigma_color, dilate, d_out_sh, d_out_valid, stream))

    def lightmap_sh_eval(self, sh, normals) -> np.ndarray:
        """mi_lightmap_sh_eval: the helper lightmap_sh_eval on the GPU, bit for bit: the irradiance E(n) [..., 3] f32 of every SH L2
        record sh [..., 9, 3] at its normal [..., 3] (check_sh_eval); an all-zero normal gives zero; not clamped.  No scene is needed."""
        S, N, shape = check_sh_eval(sh, normals)
        E = np.empty((len(N), 3), np.float32)
        abi.check(self._lib.mi_lightmap_sh_eval(self._h, len(N), S.ctypes.data, N.ctypes.data, E.ctypes.data))
        return E.reshape(shape + (3,))

    def lightmap_sh_eval_device(self, n: int, d_sh: int, d_normals: int, d_irradiance: int, stream: Optional[int] = None):
        """mi_lightmap_sh_eval_device: the same for n records held on the device (raw pointers: [n, 9, 3], [n, 3] and [n, 3] f32).
        Queued on `stream`, no synchronisation."""
        abi.check(self._lib.mi_lightmap_sh_eval_device(self._h, n, d_sh, d_normals, d_irradiance, stream))

    # ---- lightmap lookup: a finished lightmap read at uv points ----
    def lightmap_sample(self, image, uv, valid=None, flags: int = 0):
        """mi_lightmap_sample: the helper lightmap_sample on the GPU, bit for bit: `image` [H, W, 3], [H, W, 27] or [H, W, 9, 3] f32 read
        at `uv` [..., 2], bilinear over the texels `valid` ([H, W], None = all) lets take part, or with abi.MI_LS_NEAREST the reference's
        nearest texel.  Returns (out [..., C] f32, weight [...] f32).  No scene is needed."""
        return self._lookup("sample", check_lightmap_lookup(image, uv, valid, flags), None, chain_args=False)

    def _lookup(self, name, checked, lod, sh=False, stored=None, fmt=None, chain_args=True, channels_arg=True):
        """One host lookup through mi_lightmap_<name>: the buffers, None as NULL, the call, the reshape.  `checked`: what
        check_lightmap_lookup (lod None: level 0 alone) or check_lightmap_lod returned; `stored`: the levels as the call reads them where
        they are not the f32 levels checked (packed texels, blocks); `fmt`: the packed calls' format argument; chain_args: the call
        takes levels, mips, mip_valid and lod (all but the two level-0 calls); channels_arg: a plain call takes a channel count (all
        but BC6H's)."""
        if lod is None:
            img, T, v0, flags, N, shape = checked
            stored, L, mips, mv, D = stored or [img], 1, None, None, None
        else:
            levels, masks, T, D, N, shape = checked
            stored, img, flags, L = stored or levels, levels[0], 0, len(levels)
            v0 = None if masks[0] is None else np.ascontiguousarray(masks[0], np.uint8)
            mv = None if L < 2 or masks[1] is None else _lmm_pack(masks, np.uint8)
            mips = _lmm_pack(stored, stored[0].dtype, stored[0].shape[2:])
        H, W, ch = img.shape
        out = np.empty((len(T), 3 if sh else ch), np.float32)
        weight = np.empty(len(T), np.float32)
        ptr = lambda a: None if a is None else a.ctypes.data
        args = (() if fmt is None else (fmt,)) + (W, H) + ((ch,) if channels_arg and not sh else ()) + (stored[0].ctypes.data, ptr(v0))
        args += ((L, ptr(mips), ptr(mv)) if chain_args else ()) + (len(T), T.ctypes.data) + ((N.ctypes.data,) if sh else ())
        args += ((ptr(D),) if chain_args else ()) + (flags, out.ctypes.data, weight.ctypes.data)
        abi.check(getattr(self._lib, "mi_lightmap_" + name)(self._h, *args))
        return out.reshape(shape + out.shape[1:]), weight.reshape(shape)

    def lightmap_sample_device(self, width: int, height: int, channels: int, d_image: int, n: int, d_uv: int, d_out: int,
                               d_weight: Optional[int] = None, d_valid: Optional[int] = None, flags: int = 0,
                               stream: Optional[int] = None):
        """mi_lightmap_sample_device: the same for an image and points held on the device (raw pointers: [H, W, channels] f32, an optional
        [H, W] u8 mask, [n, 2] f32 in; [n, channels] f32 and an optional [n] f32 out, which must not overlap the inputs).  Queued on
        `stream`, no synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_sample_device(self._h, width, height, channels, d_image, d_valid, n, d_uv, flags, d_out, d_weight,
                                                      stream))

    def lightmap_sh_sample(self, sh, uv, normals, valid=None, flags: int = 0):
        """mi_lightmap_sh_sample: the helper lightmap_sh_sample on the GPU, bit for bit: the irradiance of a finished directional
        lightmap `sh` [H, W, 9, 3] f32 at `uv` [..., 2] for the normals [..., 3] there (mi_intersect_rays' out_uv and out_normal go in as
        they stand).  Returns (E [..., 3] f32, weight [...] f32).  No scene is needed."""
        if normals is None:
            raise ValueError("normals are required")
        checked = check_lightmap_lookup(sh, uv, valid, flags, normals)
        if checked[0].shape[2] != 27:
            raise ValueError(f"sh must be [H, W, 9, 3] or [H, W, 27], got {np.shape(sh)}")
        return self._lookup("sh_sample", checked, None, sh=True, chain_args=False)

    def lightmap_sh_sample_device(self, width: int, height: int, d_sh: int, n: int, d_uv: int, d_normals: int, d_irradiance: int,
                                  d_weight: Optional[int] = None, d_valid: Optional[int] = None, flags: int = 0,
                                  stream: Optional[int] = None):
        """mi_lightmap_sh_sample_device: the same for records and points held on the device (raw pointers: [H, W, 9, 3] f32, an optional
        [H, W] u8 mask, [n, 2] and [n, 3] f32 in; [n, 3] f32 and an optional [n] f32 out).  Queued on `stream`, no synchronisation."""
        abi.check(self._lib.mi_lightmap_sh_sample_device(self._h, width, height, d_sh, d_valid, n, d_uv, d_normals, flags, d_irradiance,
                                                         d_weight, stream))

    # ---- lightmap mips: the coverage-aware pyramid and the trilinear lookups ----
    def lightmap_mips(self, image, valid=None, levels: int = 0, want_valid: bool = True, want_coverage: bool = True):
        """mi_lightmap_mips: the helper lightmap_mips on the GPU, bit for bit: the coverage-aware mip chain of `image` [H, W, 3],
        [H, W, 27] or [H, W, 9, 3] f32 under `valid` ([H, W], None = all).  Returns the helper's three per-level lists (mips, valids,
        coverage), level 0 being the inputs themselves; without want_valid / want_coverage that plane is not asked for (out_valid /
        out_coverage NULL) and its list is None.  No scene is needed."""
        img, v8, layout = check_lightmap_mips(image, valid, levels)
        H, W, ch = img.shape
        total = sum(w * h for w, h, _ in layout[1:])
        mips = np.empty((max(total, 1), ch), np.float32)
        mv = np.empty(max(total, 1), np.uint8) if want_valid else None
        cov = np.empty(max(total, 1), np.float32) if want_coverage else None
        abi.check(self._lib.mi_lightmap_mips(self._h, W, H, ch, img.ctypes.data, None if v8 is None else v8.ctypes.data, len(layout),
                                             mips.ctypes.data, None if mv is None else mv.ctypes.data,
                                             None if cov is None else cov.ctypes.data))
        ok = np.ones((H, W), np.uint8) if v8 is None else v8

        def split(flat, first, tail=()):
            return None if flat is None else [first] + [flat[o:o + w * h].reshape((h, w) + tail) for w, h, o in layout[1:]]
        return split(mips, img, (ch,)), split(mv, ok), split(cov, np.where(ok != 0, np.float32(1.0), np.float32(0.0)))

    def lightmap_mips_device(self, width: int, height: int, channels: int, d_image: int, levels: int, d_mips: int,
                             d_mip_valid: Optional[int] = None, d_mip_coverage: Optional[int] = None, d_valid: Optional[int] = None,
                             stream: Optional[int] = None):
        """mi_lightmap_mips_device: the same for an image held on the device (raw pointers: [H, W, channels] f32 and an optional [H, W] u8
        mask in; levels 1 .. L - 1 tightly packed as lightmap_mip_layout lays them out: [sum W_l H_l, channels] f32, and optionally
        [sum W_l H_l] u8 and f32, out, which must not overlap the inputs).  Queued on `stream`, no synchronisation.  Without
        d_mip_coverage the coverage planes live in a buffer the context owns: two such calls must not be in flight at once."""
        abi.check(self._lib.mi_lightmap_mips_device(self._h, width, height, channels, d_image, d_valid, levels, d_mips, d_mip_valid,
                                                    d_mip_coverage, stream))

    def lightmap_sample_lod(self, chain, uv, lod, valid_chain=None, flags: int = 0):
        """mi_lightmap_sample_lod: the helper lightmap_sample_lod on the GPU, bit for bit: the chain lightmap_mips returned (levels and
        masks, per level) read at `uv` [..., 2] and `lod` (a scalar or uv's leading shape), trilinear over the valid texels.  Returns
        (out [..., C] f32, weight [...] f32).  No scene is needed."""
        return self._lookup("sample_lod", check_lightmap_lod(chain, uv, lod, valid_chain, flags), lod)

    def lightmap_sample_lod_device(self, width: int, height: int, channels: int, d_image: int, levels: int, d_mips: Optional[int], n: int,
                                   d_uv: int, d_lod: int, d_out: int, d_weight: Optional[int] = None, d_valid: Optional[int] = None,
                                   d_mip_valid: Optional[int] = None, flags: int = 0, stream: Optional[int] = None):
        """mi_lightmap_sample_lod_device: the same for a chain and points held on the device (raw pointers: level 0 [H, W, channels] f32
        and its optional mask, levels 1 .. L - 1 packed as mi_lightmap_mips_device writes them with their optional masks, [n, 2] and
        [n] f32 in; [n, channels] f32 and an optional [n] f32 out).  Queued on `stream`, no synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_sample_lod_device(self._h, width, height, channels, d_image, d_valid, levels, d_mips, d_mip_valid,
                                                          n, d_uv, d_lod, flags, d_out, d_weight, stream))

    def lightmap_sh_sample_lod(self, chain, uv, normals, lod, valid_chain=None, flags: int = 0):
        """mi_lightmap_sh_sample_lod: the helper lightmap_sh_sample_lod on the GPU, bit for bit: the irradiance of a directional
        lightmap's mip chain at `uv` [..., 2], the normals [..., 3] there and `lod`.  Returns (E [..., 3] f32, weight [...] f32)."""
        if normals is None:
            raise ValueError("normals are required")
        checked = check_lightmap_lod(chain, uv, lod, valid_chain, flags, normals)
        if checked[0][0].shape[2] != 27:
            raise ValueError(f"the levels must be [H, W, 9, 3] or [H, W, 27], got {np.shape(chain[0])}")
        return self._lookup("sh_sample_lod", checked, lod, sh=True)

    def lightmap_sh_sample_lod_device(self, width: int, height: int, d_sh: int, levels: int, d_mips: Optional[int], n: int, d_uv: int,
                                      d_normals: int, d_lod: int, d_irradiance: int, d_weight: Optional[int] = None,
                                      d_valid: Optional[int] = None, d_mip_valid: Optional[int] = None, flags: int = 0,
                                      stream: Optional[int] = None):
        """mi_lightmap_sh_sample_lod_device: the same for records and points held on the device (raw pointers as
        lightmap_sample_lod_device at 27 channels, and [n, 3] f32 normals in; [n, 3] f32 and an optional [n] f32 out).  Queued on
        `stream`, no synchronisation."""
        abi.check(self._lib.mi_lightmap_sh_sample_lod_device(self._h, width, height, d_sh, d_valid, levels, d_mips, d_mip_valid, n, d_uv,
                                                             d_normals, d_lod, flags, d_irradiance, d_weight, stream))

    # ---- packed lightmaps: f16 / RGB9E5 storage and the lookups that read it ----
    def lightmap_pack(self, texels, format):
        """mi_lightmap_pack: the helper lightmap_pack on the GPU, bit for bit: `texels` [..., 3] or [..., 27] f32 as uint16 [..., C]
        (abi.MI_LP_F16) or uint32 [...] (abi.MI_LP_RGB9E5, 3 channels).  No scene is needed."""
        x = np.ascontiguousarray(np.asarray(texels, np.float32))
        if x.ndim < 1 or x.shape[-1] not in (3, 27):
            raise ValueError(f"texels must be [..., 3] or [..., 27], got {x.shape}")
        ch = x.shape[-1]
        fmt = _check_packed_format(format, ch)
        out = np.empty(x.shape, np.uint16) if fmt == abi.MI_LP_F16 else np.empty(x.shape[:-1], np.uint32)
        abi.check(self._lib.mi_lightmap_pack(self._h, fmt, ch, x.size // ch, x.ctypes.data, out.ctypes.data))
        return out

    def lightmap_pack_device(self, format: int, channels: int, n_texels: int, d_texels: int, d_packed: int, stream: Optional[int] = None):
        """mi_lightmap_pack_device: the same for texels held on the device (raw pointers: [n_texels, channels] f32 in; [n_texels, channels]
        u16 or [n_texels] u32 out, which must not overlap the input).  Queued on `stream`, no synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_pack_device(self._h, format, channels, n_texels, d_texels, d_packed, stream))

    def lightmap_unpack(self, packed, format):
        """mi_lightmap_unpack: the helper lightmap_unpack on the GPU, bit for bit (a NaN is a NaN): uint16 [..., C] or uint32 [...] as
        f32 [..., C]."""
        fmt, p = _check_packed_array(packed, format)
        ch = 3 if fmt == abi.MI_LP_RGB9E5 else p.shape[-1]
        n = p.size if fmt == abi.MI_LP_RGB9E5 else p.size // ch
        out = np.empty((p.shape if fmt == abi.MI_LP_RGB9E5 else p.shape[:-1]) + (ch,), np.float32)
        abi.check(self._lib.mi_lightmap_unpack(self._h, fmt, ch, n, p.ctypes.data, out.ctypes.data))
        return out

    def lightmap_unpack_device(self, format: int, channels: int, n_texels: int, d_packed: int, d_texels: int, stream: Optional[int] = None):
        """mi_lightmap_unpack_device: the same for packed texels held on the device (raw pointers).  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_unpack_device(self._h, format, channels, n_texels, d_packed, d_texels, stream))

    def lightmap_sample_packed(self, packed_chain, format, uv, lod=None, valid_chain=None, flags: int = 0):
        """mi_lightmap_sample_packed: the helper lightmap_sample_packed on the GPU, bit for bit: packed levels (a list as lightmap_pack
        returns them per level, or one array) read at `uv` [..., 2], trilinearly at `lod`, or with lod None level 0 alone (bilinear or
        abi.MI_LS_NEAREST).  Returns (out [..., C] f32, weight [...] f32)."""
        packed, checked = check_lightmap_packed(packed_chain, format, uv, lod, valid_chain, flags)
        return self._lookup("sample_packed", checked, lod, stored=packed, fmt=int(format))

    def lightmap_sample_packed_device(self, format: int, width: int, height: int, channels: int, d_image: int, levels: int,
                                      d_mips: Optional[int], n: int, d_uv: int, d_lod: Optional[int], d_out: int,
                                      d_weight: Optional[int] = None, d_valid: Optional[int] = None, d_mip_valid: Optional[int] = None,
                                      flags: int = 0, stream: Optional[int] = None):
        """mi_lightmap_sample_packed_device: the same for packed levels and points held on the device (raw pointers as
        lightmap_sample_lod_device, the texels packed; d_lod None: level 0 alone, levels 1, d_mips None).  Queued on `stream`, no
        synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_sample_packed_device(self._h, format, width, height, channels, d_image, d_valid, levels, d_mips,
                                                             d_mip_valid, n, d_uv, d_lod, flags, d_out, d_weight, stream))

    def lightmap_sh_sample_packed(self, packed_chain, format, uv, normals, lod=None, valid_chain=None, flags: int = 0):
        """mi_lightmap_sh_sample_packed: the helper lightmap_sh_sample_packed on the GPU, bit for bit: the irradiance of a directional
        lightmap packed as abi.MI_LP_F16 at `uv`, the normals there and `lod` (None: level 0 alone).  Returns (E [..., 3], weight [...])."""
        packed, checked = check_lightmap_packed(packed_chain, format, uv, lod, valid_chain, flags, normals, sh=True)
        return self._lookup("sh_sample_packed", checked, lod, sh=True, stored=packed, fmt=int(format))

    def lightmap_sh_sample_packed_device(self, format: int, width: int, height: int, d_sh: int, levels: int, d_mips: Optional[int], n: int,
                                         d_uv: int, d_normals: int, d_lod: Optional[int], d_irradiance: int,
                                         d_weight: Optional[int] = None, d_valid: Optional[int] = None,
                                         d_mip_valid: Optional[int] = None, flags: int = 0, stream: Optional[int] = None):
        """mi_lightmap_sh_sample_packed_device: the same for packed records and points held on the device.  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_sh_sample_packed_device(self._h, format, width, height, d_sh, d_valid, levels, d_mips, d_mip_valid,
                                                                n, d_uv, d_normals, d_lod, flags, d_irradiance, d_weight, stream))

    # ---- BC6H lightmaps: the block encoder, the decoder, the lookup that reads blocks ----
    def lightmap_bc6h_encode(self, image, valid=None, rounds: int = 2):
        """mi_lightmap_bc6h_encode: the helper lightmap_bc6h_encode on the GPU, byte for byte: `image` [H, W, 3] f32 (one level) as uint8
        [BH, BW, 16] blocks; `valid` None or [H, W]; `rounds` 0 .. 4.  No scene is needed."""
        img, v8, rounds = check_lightmap_bc6h_image(image, valid, rounds)
        H, W = img.shape[:2]
        out = np.empty(((H + 3) >> 2, (W + 3) >> 2, 16), np.uint8)
        abi.check(self._lib.mi_lightmap_bc6h_encode(self._h, W, H, img.ctypes.data, None if v8 is None else v8.ctypes.data, rounds, out.ctypes.data))
        return out

    def lightmap_bc6h_encode_device(self, width: int, height: int, d_image: int, d_blocks: int, rounds: int = 2, d_valid: Optional[int] = None,
                                    stream: Optional[int] = None):
        """mi_lightmap_bc6h_encode_device: the same for a level held on the device (raw pointers: [height, width, 3] f32 in, the 16-byte
        aligned blocks out, which must not overlap the inputs).  Queued on `stream`, no synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_bc6h_encode_device(self._h, width, height, d_image, d_valid, rounds, d_blocks, stream))

    def lightmap_bc6h_decode(self, blocks, width: int, height: int):
        """mi_lightmap_bc6h_decode: the helper lightmap_bc6h_decode on the GPU, bit for bit: uint8 [BH, BW, 16] as f32 [height, width, 3]."""
        b = _check_bc6h_blocks(blocks, width, height)
        out = np.empty((int(height), int(width), 3), np.float32)
        abi.check(self._lib.mi_lightmap_bc6h_decode(self._h, int(width), int(height), b.ctypes.data, out.ctypes.data))
        return out

    def lightmap_bc6h_decode_device(self, width: int, height: int, d_blocks: int, d_image: int, stream: Optional[int] = None):
        """mi_lightmap_bc6h_decode_device: the same for blocks held on the device (raw pointers).  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_bc6h_decode_device(self._h, width, height, d_blocks, d_image, stream))

    def lightmap_bc6h_chain(self, chain, valid_chain=None, rounds: int = 2):
        """The helper lightmap_bc6h_chain on the GPU: one mi_lightmap_bc6h_encode call per level of a lightmap_mips chain, each with its
        own mask.  Returns the list of uint8 [BH_l, BW_l, 16]."""
        chain = list(chain) if isinstance(chain, (list, tuple)) else [chain]
        masks = [None] * len(chain) if valid_chain is None else list(valid_chain)
        if len(masks) != len(chain):
            raise ValueError(f"valid_chain must be None or a list of {len(chain)} masks")
        return [self.lightmap_bc6h_encode(a, m, rounds) for a, m in zip(chain, masks)]

    def lightmap_sample_bc6h(self, blocks_chain, width: int, height: int, uv, lod=None, valid_chain=None, flags: int = 0):
        """mi_lightmap_sample_bc6h: the helper lightmap_sample_bc6h on the GPU, bit for bit: BC6H levels (a list as lightmap_bc6h_chain
        returns it, or one array) of a width x height lightmap read at `uv` [..., 2], trilinearly at `lod`, or with lod None level 0 alone
        (bilinear or abi.MI_LS_NEAREST).  Returns (out [..., 3] f32, weight [...] f32)."""
        blocks, checked = check_lightmap_bc6h(blocks_chain, width, height, uv, lod, valid_chain, flags)
        return self._lookup("sample_bc6h", checked, lod, stored=blocks, channels_arg=False)

    def lightmap_sample_bc6h_device(self, width: int, height: int, d_image_blocks: int, levels: int, d_mip_blocks: Optional[int], n: int,
                                    d_uv: int, d_lod: Optional[int], d_out: int, d_weight: Optional[int] = None, d_valid: Optional[int] = None,
                                    d_mip_valid: Optional[int] = None, flags: int = 0, stream: Optional[int] = None):
        """mi_lightmap_sample_bc6h_device: the same for blocks and points held on the device (raw pointers as
        lightmap_sample_packed_device, the texels in 16-byte aligned blocks; d_lod None: level 0 alone, levels 1, d_mip_blocks None).
        Queued on `stream`, no synchronisation, no scratch."""
        abi.check(self._lib.mi_lightmap_sample_bc6h_device(self._h, width, height, d_image_blocks, d_valid, levels, d_mip_blocks, d_mip_valid, n,
                                                           d_uv, d_lod, flags, d_out, d_weight, stream))

    def last_reduce_psh_ms(self) -> float:
        """Sum of the wf_reduce_psh launch durations (ms) of the last render: entry 7 of mi_last_pipeline_ms after render_points_sh /
        render_points_sh_device / bake_lightmap_sh (the entry wf_reduce_sh and wf_reduce_m2 have after their renders)."""
        return self.last_reduce_sh_ms()

    # ---- lightmap variance: second moments of a bake, and the finish they guide ----
    def render_points_moments(self, cam: Camera, points, normals, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
                              flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points_moments: render_points with the per-texel mean of squares of the samples as a further output.  Returns
        (m2 [H, W, 3] f32, f32, u8, sig, stats): m2 sums v * v in sample order in f32 and divides by aa_sample_count, as the mean does;
        the rest is what render_points returns, bit for bit."""
        p, n, rows = check_point_table(cam, points, normals)
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        m2 = np.empty((H, W, 3), np.float32)
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_render_points_moments(
            self._h, C.byref(pod), C.byref(opts), p.ctypes.data, n.ctypes.data, rows, m2.ctypes.data,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None, C.byref(st)))
        return m2, f32, u8, sig, st

    def render_points_moments_device(self, cam: Camera, d_points: int, d_normals: int, rows_per_pixel: int,
                                     d_compact_m2: Optional[int] = None, d_compact: Optional[int] = None, d_sig: Optional[int] = None,
                                     sample_begin: int = 0, sample_end: Optional[int] = None, d_accum: Optional[int] = None, seed: int = 1,
                                     rank: int = 0, world: int = 1, stream: Optional[int] = None, flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points_moments_device: render_points_device with d_compact_m2, [compact_size(...)[1] * 1024, 3] float32 in the
        compact layout (unpermute_device un-permutes it), the moments output and their running accumulator across progressive calls
        (started by the call with sample_begin == 0, divided by the one that reaches aa_sample_count); None is exactly
        render_points_device."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=abi.MI_VARIANT_DEFAULT,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        end = cam.aa_sample_count if sample_end is None else sample_end
        abi.check(self._lib.mi_render_points_moments_device(self._h, C.byref(pod), C.byref(opts), d_points, d_normals, rows_per_pixel,
                                                            sample_begin, end, d_accum, d_compact_m2, d_compact, d_sig, stream, C.byref(st)))
        return st

    def bake_lightmap_moments(self, cam: Camera, mesh, jitter: bool = True, offset: float = 1e-3, seed: int = 1, transform=None,
                              want_f32=True, want_u8=True, want_sig=False, want_triangle=False, flags: int = 0, max_state_bytes: int = 0):
        """mi_bake_lightmap_moments: bake_lightmap with the second moments.  Returns (m2 [H, W, 3] f32, f32, u8, sig, triangle, stats);
        everything behind m2 is what bake_lightmap returns, bit for bit."""
        pod, keep = mesh_pod(mesh, transform)
        cpod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        m2 = np.empty((H, W, 3), np.float32)
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        tri = np.empty((cam.aa_sample_count if jitter else 1, H, W), np.int32) if want_triangle else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_bake_lightmap_moments(
            self._h, C.byref(cpod), C.byref(opts), C.byref(pod), abi.MI_LM_JITTER if jitter else 0, offset, m2.ctypes.data,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None,
            tri.ctypes.data if tri is not None else None, C.byref(st)))
        del keep
        return m2, f32, u8, sig, tri, st

    def lightmap_finish_var(self, image, m2, samples: int, points, normals, levels: int = 3, normal_power_log2: int = 5,
                            sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = 8.0,
                            color_floor: float = 1e-6, dilate: int = 4):
        """mi_lightmap_finish_var: the helper lightmap_finish_var on the GPU, bit for bit.  `image` and `m2` are a bake's mean and
        second moments [H, W, 3] f32 (bake_lightmap_moments), `samples` its sample count, `points` and `normals` the atlas's centre table
        ([H, W, 3], or lightmap_texels' [1, H, W, 3]).  Returns (out [H, W, 3] f32, var [H, W] f32, valid [H, W] bool).  No scene is
        needed."""
        img, P, N = check_finish_tables(image, _centre_table(points), _centre_table(normals))
        M2 = np.ascontiguousarray(m2, np.float32)
        if M2.shape != img.shape:
            raise ValueError(f"m2 must have the image's shape {img.shape}, got {M2.shape}")
        H, W = img.shape[:2]
        out = np.empty((H, W, 3), np.float32)
        var = np.empty((H, W), np.float32)
        valid = np.empty((H, W), np.uint8)
        abi.check(self._lib.mi_lightmap_finish_var(self._h, W, H, img.ctypes.data, M2.ctypes.data, samples, P.ctypes.data, N.ctypes.data,
                                                   levels, normal_power_log2, sigma_plane, reach, sigma_color, color_floor, dilate,
                                                   out.ctypes.data, var.ctypes.data, valid.ctypes.data))
        return out, var, valid.astype(bool)

    def lightmap_finish_var_device(self, width: int, height: int, d_image: int, d_m2: int, samples: int, d_points: int, d_normals: int,
                                   d_out_image: int, d_out_var: Optional[int] = None, d_out_valid: Optional[int] = None, levels: int = 3,
                                   normal_power_log2: int = 5, sigma_plane: float = float("inf"), reach: float = float("inf"),
                                   sigma_color: float = 8.0, color_floor: float = 1e-6, dilate: int = 4, stream: Optional[int] = None):
        """mi_lightmap_finish_var_device: the same for tables held on the device (raw pointers, e.g. tensor.data_ptr(): four [H, W, 3]
        f32 inputs, the [H, W, 3] f32 output and the optional [H, W] f32 variance, which must overlap none of them, and an optional
        [H, W] u8 mask).  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_finish_var_device(self._h, width, height, d_image, d_m2, samples, d_points, d_normals, levels,
                                                          normal_power_log2, sigma_plane, reach, sigma_color, color_floor, dilate,
                                                          d_out_image, d_out_var, d_out_valid, stream))

    # ---- adaptive lightmap bake: select, gather, merge, the finish with counts, the whole bake ----
    def lightmap_select(self, image, m2, counts, normals, target_rel: float, target_abs: float, capacity: Optional[int] = None,
                        want_error: bool = True):
        """mi_lightmap_select: the helper lightmap_select on the GPU, bit for bit.  Returns (index uint32 [min(count, capacity)], count,
        error [H, W] f32 | None).  capacity None: W * H.  No scene is needed."""
        img, M2, N = check_finish_tables(image, m2, _centre_table(normals))
        cnt = check_counts_plane(counts, img.shape[:2])
        H, W = img.shape[:2]
        cap = H * W if capacity is None else int(capacity)
        index = np.empty(min(cap, H * W), np.uint32)
        count = C.c_uint32(0)
        err = np.empty((H, W), np.float32) if want_error else None
        abi.check(self._lib.mi_lightmap_select(self._h, W, H, img.ctypes.data, M2.ctypes.data, cnt.ctypes.data, N.ctypes.data, target_rel,
                                               target_abs, cap, index.ctypes.data if index.size else None, C.addressof(count),
                                               err.ctypes.data if err is not None else None))
        return index[:min(count.value, cap)].copy(), int(count.value), err

    def lightmap_select_device(self, width: int, height: int, d_image: int, d_m2: int, d_counts: int, d_normals: int, target_rel: float,
                               target_abs: float, capacity: int, d_out_index: Optional[int], d_out_count: int,
                               d_out_error: Optional[int] = None, stream: Optional[int] = None):
        """mi_lightmap_select_device: the same for planes held on the device (raw pointers: [H, W, 3] f32 image, m2 and normals, [H, W]
        u32 counts; outputs: `capacity` u32, one u32, an optional [H, W] f32 plane).  Queued on `stream`; entries at and behind
        min(count, capacity) are not written."""
        abi.check(self._lib.mi_lightmap_select_device(self._h, width, height, d_image, d_m2, d_counts, d_normals, target_rel, target_abs,
                                                      capacity, d_out_index, d_out_count, d_out_error, stream))

    def lightmap_gather(self, index, points, normals, cw: int = 1024):
        """mi_lightmap_gather: the helper lightmap_gather on the GPU.  Returns the compact (points, normals) [rows, ch, cw, 3] f32."""
        idx = _check_index_list(index)
        P, N = (np.ascontiguousarray(t[None] if np.ndim(t) == 3 else t) for t in (points, normals))
        if P.dtype != np.float32 or N.dtype != np.float32 or P.ndim != 4 or P.shape[3] != 3 or P.shape != N.shape:
            raise ValueError("points and normals must be float32 [rows, H, W, 3] arrays of one shape")
        rows, H, W = P.shape[:3]
        cw = int(cw)
        ch = (idx.size + cw - 1) // cw if cw > 0 else 0
        cp = np.empty((rows, ch, max(cw, 0), 3), np.float32)
        cn = np.empty((rows, ch, max(cw, 0), 3), np.float32)
        abi.check(self._lib.mi_lightmap_gather(self._h, W, H, rows, idx.size, idx.ctypes.data, P.ctypes.data, N.ctypes.data, cw,
                                               cp.ctypes.data, cn.ctypes.data))
        return cp, cn

    def lightmap_gather_device(self, width: int, height: int, rows: int, n: int, d_index: int, d_points: int, d_normals: int, cw: int,
                               d_out_points: int, d_out_normals: int, stream: Optional[int] = None):
        """mi_lightmap_gather_device: the same for a list and tables held on the device; the outputs are [rows, ceil(n / cw), cw, 3] f32."""
        abi.check(self._lib.mi_lightmap_gather_device(self._h, width, height, rows, n, d_index, d_points, d_normals, cw, d_out_points,
                                                      d_out_normals, stream))

    def lightmap_merge(self, index, mean, m2_round, round_samples: int, image, m2, counts):
        """mi_lightmap_merge: the helper lightmap_merge on the GPU, bit for bit.  Returns new (image, m2, counts uint32); the arguments
        are not modified."""
        idx = _check_index_list(index)
        img, M2, _ = check_finish_tables(image, m2, m2)
        img, M2 = img.copy(), M2.copy()
        cnt = check_counts_plane(counts, img.shape[:2]).copy()
        mr, m2r = np.ascontiguousarray(mean, np.float32).reshape(-1), np.ascontiguousarray(m2_round, np.float32).reshape(-1)
        if mr.size < 3 * idx.size or m2r.size < 3 * idx.size:
            raise ValueError(f"mean and m2_round must hold at least {idx.size} triples")
        H, W = img.shape[:2]
        abi.check(self._lib.mi_lightmap_merge(self._h, W, H, idx.size, idx.ctypes.data, mr.ctypes.data, m2r.ctypes.data, round_samples,
                                              img.ctypes.data, M2.ctypes.data, cnt.ctypes.data))
        return img, M2, cnt

    def lightmap_merge_device(self, width: int, height: int, n: int, d_index: int, d_mean: int, d_m2_round: int, round_samples: int,
                              d_image: int, d_m2: int, d_counts: int, stream: Optional[int] = None):
        """mi_lightmap_merge_device: the same in place on planes held on the device.  Queued on `stream`."""
        abi.check(self._lib.mi_lightmap_merge_device(self._h, width, height, n, d_index, d_mean, d_m2_round, round_samples, d_image, d_m2,
                                                     d_counts, stream))

    def lightmap_finish_var_counts(self, image, m2, counts, points, normals, levels: int = 3, normal_power_log2: int = 5,
                                   sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = 8.0,
                                   color_floor: float = 1e-6, dilate: int = 4):
        """mi_lightmap_finish_var_counts: lightmap_finish_var(samples=counts plane) on the GPU, bit for bit: the variance-guided finish of
        an adaptive bake, whose texels have counts of their own.  Returns (out, var, valid) as lightmap_finish_var does."""
        img, P, N = check_finish_tables(image, _centre_table(points), _centre_table(normals))
        M2 = np.ascontiguousarray(m2, np.float32)
        if M2.shape != img.shape:
            raise ValueError(f"m2 must have the image's shape {img.shape}, got {M2.shape}")
        cnt = check_counts_plane(counts, img.shape[:2])
        H, W = img.shape[:2]
        out = np.empty((H, W, 3), np.float32)
        var = np.empty((H, W), np.float32)
        valid = np.empty((H, W), np.uint8)
        abi.check(self._lib.mi_lightmap_finish_var_counts(self._h, W, H, img.ctypes.data, M2.ctypes.data, cnt.ctypes.data, P.ctypes.data,
                                                          N.ctypes.data, levels, normal_power_log2, sigma_plane, reach, sigma_color,
                                                          color_floor, dilate, out.ctypes.data, var.ctypes.data, valid.ctypes.data))
        return out, var, valid.astype(bool)

    def lightmap_finish_var_counts_device(self, width: int, height: int, d_image: int, d_m2: int, d_counts: int, d_points: int,
                                          d_normals: int, d_out_image: int, d_out_var: Optional[int] = None,
                                          d_out_valid: Optional[int] = None, levels: int = 3, normal_power_log2: int = 5,
                                          sigma_plane: float = float("inf"), reach: float = float("inf"), sigma_color: float = 8.0,
                                          color_floor: float = 1e-6, dilate: int = 4, stream: Optional[int] = None):
        """mi_lightmap_finish_var_counts_device: lightmap_finish_var_device with a [H, W] u32 counts plane in the place of `samples`."""
        abi.check(self._lib.mi_lightmap_finish_var_counts_device(self._h, width, height, d_image, d_m2, d_counts, d_points, d_normals,
                                                                 levels, normal_power_log2, sigma_plane, reach, sigma_color, color_floor,
                                                                 dilate, d_out_image, d_out_var, d_out_valid, stream))

    def bake_lightmap_adaptive(self, cam: Camera, mesh, first_samples: int, round_samples: int, max_rounds: int, target_rel: float,
                               target_abs: float, jitter: bool = True, offset: float = 1e-3, seed: int = 1, transform=None, want_f32=True,
                               want_u8=True, want_sig=False, want_triangle=False, flags: int = 0, max_state_bytes: int = 0):
        """mi_bake_lightmap_adaptive: bake_lightmap_moments at `first_samples`, then up to `max_rounds` rounds of `round_samples` further
        samples for the texels lightmap_select picks with the two targets (cam.aa_sample_count is ignored).  Returns (counts [H, W]
        uint32, m2, f32, u8, sig, triangle, stats): the merged mean and moments and the samples behind each texel; sig and triangle are
        round 0's.  Bit for bit the composition of bake_lightmap_moments, lightmap_select, lightmap_gather, render_points_moments (seed
        + r) and lightmap_merge."""
        pod, keep = mesh_pod(mesh, transform)
        cpod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        ad = abi.mi_lightmap_adaptive(first_samples=first_samples, round_samples=round_samples, max_rounds=max_rounds,
                                      target_rel=target_rel, target_abs=target_abs)
        H, W = cam.screen_height, cam.screen_width
        counts = np.empty((H, W), np.uint32)
        m2 = np.empty((H, W, 3), np.float32)
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        tri = np.empty((max(int(first_samples), 0) if jitter else 1, H, W), np.int32) if want_triangle else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_bake_lightmap_adaptive(
            self._h, C.byref(cpod), C.byref(opts), C.byref(pod), abi.MI_LM_JITTER if jitter else 0, offset, C.byref(ad),
            counts.ctypes.data, m2.ctypes.data,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None,
            tri.ctypes.data if tri is not None else None, C.byref(st)))
        del keep
        return counts, m2, f32, u8, sig, tri, st

    def probe_volume_sample(self, volume: "ProbeVolume", points, normals, flags: int = 0):
        """mi_probe_volume_sample: the helper probe_volume_sample on the GPU, bit for bit.  `volume` is a ProbeVolume, points and
        normals [..., 3] f32 of one shape (check_volume_points).  Returns (E [..., 3] f32, weight [...] f32).  No scene is needed."""
        lo, hi, cnt, sh, valid, flags = check_probe_volume(volume.lo, volume.hi, volume.counts, volume.sh, volume.valid, flags)
        P, N, shape = check_volume_points(points, normals)
        pod = abi.mi_probe_volume(lo=abi.f3(*lo.tolist()), hi=abi.f3(*hi.tolist()), counts=(C.c_uint32 * 3)(*cnt), flags=flags,
                                  sh=sh.ctypes.data, valid=valid.ctypes.data if valid is not None else None)
        E = np.empty((len(P), 3), np.float32)
        w = np.empty(len(P), np.float32)
        abi.check(self._lib.mi_probe_volume_sample(self._h, C.byref(pod), len(P), P.ctypes.data, N.ctypes.data, E.ctypes.data, w.ctypes.data))
        return E.reshape(shape + (3,)), w.reshape(shape)

    def probe_volume_sample_device(self, lo, hi, counts, d_sh: int, n_points: int, d_points: int, d_normals: int, d_irradiance: int,
                                   d_weight: Optional[int] = None, d_valid: Optional[int] = None, flags: int = 0,
                                   stream: Optional[int] = None):
        """mi_probe_volume_sample_device: the same for a volume and points held on the device (raw pointers, e.g. tensor.data_ptr():
        d_sh [n_probes, 9, 3] f32 — render_probes' sh buffer as it is —, d_valid [n_probes] u8 or None, d_points / d_normals /
        d_irradiance [n_points, 3] f32, d_weight [n_points] f32 or None).  Queued on `stream`, no synchronisation."""
        pod = abi.mi_probe_volume(lo=abi.f3(*[float(v) for v in lo]), hi=abi.f3(*[float(v) for v in hi]),
                                  counts=(C.c_uint32 * 3)(*[int(c) for c in counts]), flags=flags, sh=d_sh, valid=d_valid)
        abi.check(self._lib.mi_probe_volume_sample_device(self._h, C.byref(pod), n_points, d_points, d_normals, d_irradiance, d_weight,
                                                          stream))

    def render_probes(self, cam: Camera, points, seed: int = 1, want_f32=True, want_u8=True, want_sig=False,
                      flags: int = 0, max_state_bytes: int = 0):
        """mi_render_probes: light probes.  `points` (check_probe_table: [S, H, W, 3] or [H, W, 3] float32, S = 1 or aa_sample_count)
        holds one probe position per pixel; sample s of probe (x, y) leaves it along rand_sphere_vec from the stream
        (seed, W*H + y*W + x, s) — uniform over the whole sphere — and its path draws from (seed, y*W + x, s).  Returns
        (sh, f32, u8, sig, stats): sh [H, W, 9, 3] float32, the SH L2 radiance coefficients per colour channel (sh9_irradiance turns
        them into irradiance), then what render returns (the mean over the samples)."""
        p, rows = check_probe_table(cam, points)
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        sh = np.empty((H, W, 9, 3), np.float32)
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_render_probes(
            self._h, C.byref(pod), C.byref(opts), p.ctypes.data, rows, sh.ctypes.data,
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None, C.byref(st)))
        return sh, f32, u8, sig, st

    # ---- device-pointer building blocks (multi-GPU; pointers are ints, e.g. tensor.data_ptr()) ----
    def render_probes_device(self, cam: Camera, d_points: int, rows_per_pixel: int, d_compact_sh: Optional[int] = None,
                             d_compact: Optional[int] = None, d_sig: Optional[int] = None, sample_begin: int = 0,
                             sample_end: Optional[int] = None, d_accum: Optional[int] = None, seed: int = 1, rank: int = 0, world: int = 1,
                             stream: Optional[int] = None, flags: int = 0, max_state_bytes: int = 0):
        """mi_render_probes_device: render_points_device for a probe table held on the device (raw pointer, [rows_per_pixel, H, W, 3]
        float32); the same sample-range, accumulator and rank / world rules.  d_compact_sh, [compact_size(...)[1] * 1024, 9, 3] float32,
        is the SH output and its running accumulator across progressive calls (started by the call with sample_begin == 0, scaled by the
        one that reaches aa_sample_count); None gives the plain outputs only."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=abi.MI_VARIANT_DEFAULT,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        end = cam.aa_sample_count if sample_end is None else sample_end
        abi.check(self._lib.mi_render_probes_device(self._h, C.byref(pod), C.byref(opts), d_points, rows_per_pixel,
                                                    sample_begin, end, d_accum, d_compact_sh, d_compact, d_sig, stream, C.byref(st)))
        return st

    def render_points_device(self, cam: Camera, d_points: int, d_normals: int, rows_per_pixel: int, d_compact: Optional[int] = None,
                             d_sig: Optional[int] = None, sample_begin: int = 0, sample_end: Optional[int] = None,
                             d_accum: Optional[int] = None, seed: int = 1, rank: int = 0, world: int = 1, stream: Optional[int] = None,
                             flags: int = 0, max_state_bytes: int = 0):
        """mi_render_points_device: render_rays_device for a point table held on the device (raw pointers, [rows_per_pixel, H, W, 3]
        float32 each); the same sample-range, accumulator and rank / world rules."""
        return self._render_table_device(self._lib.mi_render_points_device, cam, d_points, d_normals, rows_per_pixel, d_compact, d_sig,
                                         sample_begin, sample_end, d_accum, seed, rank, world, stream, flags, max_state_bytes)

    def render_rays_device(self, cam: Camera, d_origins: int, d_dirs: int, rays_per_pixel: int, d_compact: Optional[int] = None,
                           d_sig: Optional[int] = None, sample_begin: int = 0, sample_end: Optional[int] = None,
                           d_accum: Optional[int] = None, seed: int = 1, rank: int = 0, world: int = 1, stream: Optional[int] = None,
                           flags: int = 0, max_state_bytes: int = 0):
        """mi_render_rays_device: render_tiles_device and render_samples_device for a ray table held on the device (raw pointers,
        [rays_per_pixel, H, W, 3] float32 each).  The default range with d_accum None is a whole render of this rank's tiles; any other
        range adds samples [sample_begin, sample_end) to the accumulator, and the call that reaches aa_sample_count writes d_compact."""
        return self._render_table_device(self._lib.mi_render_rays_device, cam, d_origins, d_dirs, rays_per_pixel, d_compact, d_sig,
                                         sample_begin, sample_end, d_accum, seed, rank, world, stream, flags, max_state_bytes)

    def _render_table_device(self, entry, cam, d_first, d_second, rows, d_compact, d_sig, sample_begin, sample_end, d_accum, seed, rank,
                             world, stream, flags, max_state_bytes):
        """mi_render_rays_device / mi_render_points_device"""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=abi.MI_VARIANT_DEFAULT,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        end = cam.aa_sample_count if sample_end is None else sample_end
        abi.check(entry(self._h, C.byref(pod), C.byref(opts), d_first, d_second, rows,
                        sample_begin, end, d_accum, d_compact, d_sig, stream, C.byref(st)))
        return st

    def render_tiles_device(self, cam: Camera, d_compact: int, d_sig: Optional[int] = None, seed: int = 1,
                            rank: int = 0, world: int = 1, stream: Optional[int] = None,
                            variant: int = abi.MI_VARIANT_DEFAULT, flags: int = 0, max_state_bytes: int = 0):
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=variant,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        abi.check(self._lib.mi_render_tiles_device(self._h, C.byref(pod), C.byref(opts), d_compact, d_sig,
                                                   stream, C.byref(st)))
        return st

    def render_samples_device(self, cam: Camera, sample_begin: int, sample_end: int, d_accum: int,
                              d_compact: Optional[int] = None, d_sig: Optional[int] = None, seed: int = 1,
                              rank: int = 0, world: int = 1, stream: Optional[int] = None,
                              flags: int = 0, max_state_bytes: int = 0):
        """mi_render_samples_device: add samples [sample_begin, sample_end) of every pixel, in order, to the
        caller-held accumulator (float4 per compact pixel).  The call that reaches aa_sample_count also
        writes the means to d_compact.  Progressive display and checkpoint / resume are built on this."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=rank, world=world, variant=abi.MI_VARIANT_DEFAULT,
                                  want_signature=int(d_sig is not None), flags=flags, max_state_bytes=max_state_bytes)
        st = abi.mi_stats()
        abi.check(self._lib.mi_render_samples_device(self._h, C.byref(pod), C.byref(opts), sample_begin, sample_end,
                                                     d_accum, d_compact, d_sig, stream, C.byref(st)))
        return st

    def unpermute_device(self, cam: Camera, world: int, d_gathered: int, d_image: int, stream: Optional[int] = None):
        pod = cam.to_pod()
        abi.check(self._lib.mi_unpermute_device(self._h, C.byref(pod), world, d_gathered, d_image, stream))

    def tonemap_device(self, cam: Camera, d_image_f32: int, d_image_u8: int, stream: Optional[int] = None):
        pod = cam.to_pod()
        abi.check(self._lib.mi_tonemap_device(self._h, C.byref(pod), d_image_f32, d_image_u8, stream))

    def reserve(self, cam: Camera, world: int = 1, max_state_bytes: int = 0):
        """Allocate the wavefront pipeline's HBM buffers ahead of the first render (mi_reserve)."""
        pod = cam.to_pod()
        abi.check(self._lib.mi_reserve(self._h, C.byref(pod), world, max_state_bytes))

    def last_pipeline_ms(self):
        """Wavefront pipeline of the last render: dict of per-kernel duration sums (ms) and launch count."""
        out = (C.c_float * 8)()
        abi.check(self._lib.mi_last_pipeline_ms(self._h, out))
        return {"wf_main_ms": float(out[0]), "wf_trav_ms": float(out[1]), "wf_reduce_ms": float(out[2]), "launches": int(out[3]),
                "wf_trav_f_ms": float(out[4]), "wf_replay_ms": float(out[5]), "wf_main_a_ms": float(out[6])}

    def last_reduce_sh_ms(self) -> float:
        """Sum of the wf_reduce_sh launch durations (ms) of the last render: entry 7 of mi_last_pipeline_ms, the SH reduction of
        render_probes / render_probes_device; 0.0 after any other render but a moments or a directional bake, whose own reductions
        (last_reduce_m2_ms, last_reduce_psh_ms) report through the same entry."""
        out = (C.c_float * 8)()
        abi.check(self._lib.mi_last_pipeline_ms(self._h, out))
        return float(out[7])

    def last_reduce_m2_ms(self) -> float:
        """Sum of the wf_reduce_m2 launch durations (ms) of the last render: entry 7 of mi_last_pipeline_ms after
        render_points_moments / render_points_moments_device / bake_lightmap_moments (the entry wf_reduce_sh has after render_probes: the
        two never run in one render); 0.0 after any other render."""
        return self.last_reduce_sh_ms()

    def last_pipeline_counts(self):
        """Path counts of the last wavefront render (mi_last_pipeline_counts), for traffic accounting."""
        out = (C.c_uint64 * 8)()
        abi.check(self._lib.mi_last_pipeline_counts(self._h, out))
        k = ["passes", "paths_a", "paths_b", "queue_entries", "sample_slots", "pixels", "segments", "dead_tile_samples"]
        return dict(zip(k, [int(v) for v in out]))

    def last_diag(self):
        """Counters of the last MI_VARIANT_VOTED_DIAG launch as a dict (diagnostic)."""
        out = (C.c_uint64 * 16)()
        abi.check(self._lib.mi_last_diag(self._h, out))
        k = ["a_trips", "a_lanes", "inner_trips", "inner_lanes", "leaf_trips", "leaf_lanes", "b_trips", "waves",
             "a_cycles", "b_cycles", "shade_cycles", "gen_cycles", "list_cycles", "slab_tests", "segments"]
        return dict(zip(k, [int(v) for v in out]))

    def selftest(self):
        """mi_selftest: exhaustive check of the kernels' short reciprocal against the IEEE division -> (mismatches, checked)."""
        out = (C.c_uint64 * 4)()
        abi.check(self._lib.mi_selftest(self._h, out))
        return int(out[0]), int(out[1])

    def last_kernel_ms(self) -> float:
        ms = C.c_float()
        abi.check(self._lib.mi_last_kernel_ms(self._h, C.byref(ms)))
        return float(ms.value)

    # ---- ray queries: Scene::intersect_ray / Scene::shade_ray for rays of the caller's making ----
    def intersect_rays(self, origins, dirs, t_min: float = 0.001, t_max: float = float("inf"), seed: int = 1,
                       first_key: int = 0, resolve: bool = True) -> RayHits:
        """mi_intersect_rays: the closest hit of every ray over Scene.objects.  Ray i draws from the stream (seed, first_key + i, 0).
        resolve=False is the visibility form: object and distance only."""
        o, d, t_min, t_max = check_rays(origins, dirs, t_min, t_max)
        n = len(o)
        r = RayHits(object=np.zeros(n, np.int32), distance=np.zeros(n, np.float32))
        flags = None
        if resolve:
            r.hitpoint, r.normal = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
            r.uv, r.material = np.zeros((n, 2), np.float32), np.zeros(n, MATERIAL_DTYPE)
            flags = np.zeros(n, np.int32)
        ptr = lambda a: a.ctypes.data if a is not None else None
        abi.check(self._lib.mi_intersect_rays(self._h, n, o.ctypes.data, d.ctypes.data, t_min, t_max, seed, first_key & 0xffffffff,
                                              ptr(r.object), ptr(r.distance), ptr(r.hitpoint), ptr(r.normal), ptr(flags), ptr(r.uv),
                                              ptr(r.material)))
        if resolve:
            r.frontface, r.has_uv = (flags & 1) != 0, (flags & 2) != 0
        return r

    def intersect_rays_device(self, n_rays: int, d_origins: int, d_dirs: int, d_object: int, d_distance: Optional[int] = None,
                              d_hitpoint: Optional[int] = None, d_normal: Optional[int] = None, d_flags: Optional[int] = None,
                              d_uv: Optional[int] = None, d_material: Optional[int] = None, t_min: float = 0.001,
                              t_max: float = float("inf"), seed: int = 1, first_key: int = 0, stream: Optional[int] = None):
        """mi_intersect_rays_device: raw device pointers (ints), one kernel queued on `stream`, no synchronisation."""
        t_min, t_max = float(t_min), float(t_max)
        if t_min != t_min or t_max != t_max:
            raise ValueError("t_min / t_max must not be NaN")
        abi.check(self._lib.mi_intersect_rays_device(self._h, n_rays, d_origins, d_dirs, t_min, t_max, seed, first_key & 0xffffffff,
                                                     d_object, d_distance, d_hitpoint, d_normal, d_flags, d_uv, d_material, stream))

    def occluded_rays(self, origins, dirs, t_min: float = 0.001, t_max: float = float("inf"), ray_t_max=None, seed: int = 1,
                      first_key: int = 0) -> np.ndarray:
        """mi_occluded_rays: for every ray, is Scene::intersect_ray(ray, t_min, t_max) Some?  -> [n] bool.  The any-hit query: a ray is
        done at its first accepted hit.  `ray_t_max` ([n] floats) replaces `t_max` ray by ray.  Directions are used as given, so the
        segment a -> b is origins = a, dirs = b - a, t_min = eps, t_max = 1 - eps.  Ray i draws from the stream (seed, first_key + i, 0)."""
        o, d, t_min, t_max = check_rays(origins, dirs, t_min, t_max)
        tm = check_ray_t_max(ray_t_max, len(o))
        out = np.zeros(len(o), np.uint8)
        abi.check(self._lib.mi_occluded_rays(self._h, len(o), o.ctypes.data, d.ctypes.data, t_min, t_max,
                                             tm.ctypes.data if tm is not None else None, seed, first_key & 0xffffffff, out.ctypes.data))
        return out != 0

    def occluded_rays_device(self, n_rays: int, d_origins: int, d_dirs: int, d_occluded: int, d_ray_t_max: Optional[int] = None,
                             t_min: float = 0.001, t_max: float = float("inf"), seed: int = 1, first_key: int = 0,
                             stream: Optional[int] = None):
        """mi_occluded_rays_device: raw device pointers (ints; d_occluded [n] bytes, d_ray_t_max [n] f32 or None), one kernel queued on
        `stream`, no synchronisation.  Only the scalars are checked: a NaN in a device ray_t_max gives an unspecified answer for that ray."""
        t_min, t_max = float(t_min), float(t_max)
        if t_min != t_min or t_max != t_max:
            raise ValueError("t_min / t_max must not be NaN")
        abi.check(self._lib.mi_occluded_rays_device(self._h, n_rays, d_origins, d_dirs, t_min, t_max, d_ray_t_max, seed,
                                                    first_key & 0xffffffff, d_occluded, stream))

    def hemisphere_occlusion(self, points, normals, n_samples: int, t_min: float = 0.001, t_max: float = float("inf"), flags: int = 0,
                             seed: int = 1, first_key: int = 0, first_sample: int = 0, want_bent: bool = True):
        """mi_hemisphere_occlusion: per surface point, how many of `n_samples` hemisphere rays about its normal are NOT occluded within
        [t_min, t_max] -> (open [n] uint32, bent [n, 3] f32 or None: the sum of the open directions).  The rays are made on the GPU:
        sample s = first_sample + k of point i takes its direction from Lambertian::scatter's sample_hemisphere on the stream
        (seed, first_key + i, 2s) and its ray draws from (seed, first_key + i, 2s + 1).  Normals and directions are used as given;
        flags = abi.MI_HEMI_WORLD_RADIUS makes t_max a world-space radius.  A bake split by points (first_key advanced) or by samples
        (first_sample advanced, counts added) gives the counts of one call exactly."""
        p, n, n_samples, t_min, t_max, flags, first_sample = check_hemisphere(points, normals, n_samples, t_min, t_max, flags, first_sample)
        out_open = np.zeros(len(p), np.uint32)
        out_bent = np.zeros((len(p), 3), np.float32) if want_bent else None
        abi.check(self._lib.mi_hemisphere_occlusion(self._h, len(p), p.ctypes.data, n.ctypes.data, first_sample, n_samples, t_min, t_max,
                                                    flags, seed, first_key & 0xffffffff, out_open.ctypes.data,
                                                    out_bent.ctypes.data if want_bent else None))
        return out_open, out_bent

    def hemisphere_occlusion_device(self, n_points: int, d_points: int, d_normals: int, d_open: int, n_samples: int,
                                    d_bent: Optional[int] = None, t_min: float = 0.001, t_max: float = float("inf"), flags: int = 0,
                                    seed: int = 1, first_key: int = 0, first_sample: int = 0, stream: Optional[int] = None):
        """mi_hemisphere_occlusion_device: raw device pointers (ints; d_points / d_normals [n][3] f32, d_open [n] uint32, d_bent [n][3]
        f32 or None), one kernel queued on `stream`, no synchronisation."""
        t_min, t_max = float(t_min), float(t_max)
        if t_min != t_min or t_max != t_max:
            raise ValueError("t_min / t_max must not be NaN")
        abi.check(self._lib.mi_hemisphere_occlusion_device(self._h, n_points, d_points, d_normals, first_sample, n_samples, t_min, t_max,
                                                           flags, seed, first_key & 0xffffffff, d_open, d_bent, stream))

    def shade_rays(self, cam: Camera, origins, dirs, seed: int = 1, first_key: int = 0) -> np.ndarray:
        """mi_shade_rays: Scene::shade_ray at level 0 for every ray -> [n, 3] f32 radiance.  `cam` supplies path_depth,
        path_samples and max_trace_dist."""
        o, d, _, _ = check_rays(origins, dirs)
        pod = check_shade_camera(cam).to_pod()
        out = np.zeros((len(o), 3), np.float32)
        abi.check(self._lib.mi_shade_rays(self._h, C.byref(pod), len(o), o.ctypes.data, d.ctypes.data, seed, first_key & 0xffffffff,
                                          out.ctypes.data))
        return out

    def shade_rays_device(self, cam: Camera, n_rays: int, d_origins: int, d_dirs: int, d_rgb: int, seed: int = 1,
                          first_key: int = 0, stream: Optional[int] = None):
        pod = check_shade_camera(cam).to_pod()
        abi.check(self._lib.mi_shade_rays_device(self._h, C.byref(pod), n_rays, d_origins, d_dirs, seed, first_key & 0xffffffff,
                                                 d_rgb, stream))


class MultiContext:
    """mi_multi: N GPUs of one node behind ONE handle (one context, stream and host thread per device inside the
    library; tiles t % N; a single RCCL send/recv fan-in per frame; un-permute and tone-map on device 0)."""

    def __init__(self, n_devices: int, devices=None, _loopback_device=None):
        self._lib = abi.load()
        self._h = C.c_void_p()
        if _loopback_device is not None:
            abi.check(self._lib.mi_multi_create_loopback(n_devices, _loopback_device, C.byref(self._h)))
        else:
            arr = (C.c_int * n_devices)(*devices) if devices is not None else None
            abi.check(self._lib.mi_multi_create(n_devices, arr, C.byref(self._h)))
        self.n_devices = n_devices

    @classmethod
    def loopback(cls, n_contexts: int, device: int = 0) -> "MultiContext":
        """mi_multi_create_loopback: the TEST transport — `n_contexts` ranks on one device, the RCCL fan-in replaced by
        event-ordered device-to-device copies; everything else is mi_multi_render's N >= 2 code."""
        return cls(n_contexts, _loopback_device=device)

    def close(self):
        if self._h:
            self._lib.mi_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, flat: FlatScene):
        abi.check(self._lib.mi_multi_scene_upload(self._h, C.byref(flat.desc)))

    def context(self, rank: int) -> Context:
        """The context of device number `rank`, borrowed (mi_multi_context): per-device timing and path counts."""
        h = self._lib.mi_multi_context(self._h, rank)
        if not h:
            abi.check(abi.MI_ERR_INVALID)
        return Context(rank, _borrowed=h)

    def reserve(self, cam: Camera, max_state_bytes: int = 0):
        pod = cam.to_pod()
        abi.check(self._lib.mi_multi_reserve(self._h, C.byref(pod), max_state_bytes))

    def render(self, cam: Camera, seed: int = 1, want_f32=True, want_u8=True, want_sig=False, flags: int = 0,
               max_state_bytes: int = 0, variant: int = abi.MI_VARIANT_DEFAULT):
        """mi_multi_render: the whole image, assembled on device 0.  Same return value as Context.render.  With no output
        wanted the finished f32 and u8 images stay resident on device 0 (nothing crosses PCIe)."""
        pod = cam.to_pod()
        opts = abi.mi_render_opts(seed=seed, rank=0, world=1, variant=variant, want_signature=int(want_sig),
                                  flags=flags, max_state_bytes=max_state_bytes)
        H, W = cam.screen_height, cam.screen_width
        f32 = np.empty((H, W, 3), np.float32) if want_f32 else None
        u8 = np.empty((H, W, 3), np.uint8) if want_u8 else None
        sig = np.empty((H, W), np.uint32) if want_sig else None
        st = abi.mi_stats()
        abi.check(self._lib.mi_multi_render(
            self._h, C.byref(pod), C.byref(opts),
            f32.ctypes.data if f32 is not None else None,
            u8.ctypes.data if u8 is not None else None,
            sig.ctypes.data if sig is not None else None, C.byref(st)))
        return f32, u8, sig, st


def compact_size(cam: Camera, world: int):
    """(tiles_total, tiles_padded) of the tile partition (mi_compact_size)."""
    pod = cam.to_pod()
    a, b = C.c_uint32(), C.c_uint32()
    abi.check(abi.load().mi_compact_size(C.byref(pod), world, C.byref(a), C.byref(b)))
    return int(a.value), int(b.value)


@dataclass
class Scene:                         # tracing.rs:213-218
    camera: Camera
    objects: List[Intersectable]
    point_light_pos: tuple = (0.0, 1.0, 5.0)    # read by ShadingMode::Phong only (tracing.rs:282,288)
    ambient: tuple = (0.1, 0.1, 0.1)            # Phong only (:292)

    def flatten(self) -> FlatScene:
        fb = FlatBuilder()
        for obj in self.objects:
            obj.flatten(fb)
        flat = fb.finish()
        flat.desc.point_light_pos = abi.f3(*[float(v) for v in self.point_light_pos])
        flat.desc.ambient = abi.f3(*[float(v) for v in self.ambient])
        return flat

    def render_to_image(self, seed: int = 1, device: int = 0) -> np.ndarray:
        """Scene::render_to_image (tracing.rs:221-263): returns the RgbImage bytes [H,W,3] u8."""
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            _, u8, _, _ = ctx.render(self.camera, seed=seed, want_f32=False, want_u8=True)
            return u8
        finally:
            ctx.close()

    def intersect_rays(self, origins, dirs, t_min: float = 0.001, t_max: float = float("inf"), seed: int = 1, first_key: int = 0,
                       resolve: bool = True, device: int = 0) -> RayHits:
        """`impl Intersectable for Scene` (tracing.rs:326-346) for a batch of rays: flatten -> upload -> one query."""
        o, d, t_min, t_max = check_rays(origins, dirs, t_min, t_max)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            return ctx.intersect_rays(o, d, t_min, t_max, seed=seed, first_key=first_key, resolve=resolve)
        finally:
            ctx.close()

    def occluded_rays(self, origins, dirs, t_min: float = 0.001, t_max: float = float("inf"), ray_t_max=None, seed: int = 1,
                      first_key: int = 0, device: int = 0) -> np.ndarray:
        """Is `Scene::intersect_ray(ray, t_min, t_max)` (tracing.rs:326-346) Some, for a batch of rays: flatten -> upload -> one query."""
        o, d, t_min, t_max = check_rays(origins, dirs, t_min, t_max)
        tm = check_ray_t_max(ray_t_max, len(o))
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            return ctx.occluded_rays(o, d, t_min, t_max, ray_t_max=tm, seed=seed, first_key=first_key)
        finally:
            ctx.close()

    def ambient_occlusion(self, points, normals, samples: int = 64, radius: float = float("inf"), t_min: float = 0.001, seed: int = 1,
                          first_key: int = 0, first_sample: int = 0, world_radius: bool = True, want_bent: bool = False, device: int = 0):
        """Ambient occlusion of surface points (mi_hemisphere_occlusion): flatten -> upload -> one query.  -> the open fraction
        `out_open / samples` per point ([n] float64 in [0, 1]; 1 = nothing within `radius`), or with want_bent (fraction, bent [n, 3]
        f32: the sum of the open directions).  `radius` is in world units (MI_HEMI_WORLD_RADIUS) unless world_radius is False, then in
        units of each direction's own length, like every t_max of the ray queries.  Offset the points off the surface yourself, or
        rely on t_min."""
        flags = abi.MI_HEMI_WORLD_RADIUS if world_radius else 0
        p, n, samples, t_min, radius, flags, first_sample = check_hemisphere(points, normals, samples, t_min, radius, flags, first_sample)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            out_open, bent = ctx.hemisphere_occlusion(p, n, samples, t_min, radius, flags, seed=seed, first_key=first_key,
                                                      first_sample=first_sample, want_bent=want_bent)
        finally:
            ctx.close()
        frac = out_open.astype(np.float64) / samples
        return (frac, bent) if want_bent else frac

    def render_rays(self, origins, dirs, seed: int = 1, device: int = 0) -> np.ndarray:
        """Scene::render_to_image (tracing.rs:221-263) with a ray table in place of Camera::generate_rays (mi_render_rays): the RgbImage
        bytes [H,W,3] u8.  This scene's camera supplies the image size, aa_sample_count, path_depth, max_trace_dist and gamma."""
        o, d, _ = check_ray_table(self.camera, origins, dirs)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            _, u8, _, _ = ctx.render_rays(self.camera, o, d, seed=seed, want_f32=False, want_u8=True)
            return u8
        finally:
            ctx.close()

    def render_points(self, points, normals, seed: int = 1, device: int = 0) -> np.ndarray:
        """A lightmap / irradiance bake (mi_render_points): the RgbImage bytes [H,W,3] u8 of the light gathered at a table of surface
        points and normals (lightmap_texels makes one from a mesh) — per texel the mean over aa_sample_count cosine-distributed
        directions of Scene::shade_ray, the directions drawn on the GPU.  This scene's camera supplies the image size, aa_sample_count,
        path_depth, max_trace_dist and gamma.  Texels with a zero normal are empty and stay black."""
        p, n, _ = check_point_table(self.camera, points, normals)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            _, u8, _, _ = ctx.render_points(self.camera, p, n, seed=seed, want_f32=False, want_u8=True)
            return u8
        finally:
            ctx.close()

    def bake_lightmap(self, mesh, width: int, height: int, samples: int, jitter: bool = True, offset: float = 1e-3, seed: int = 1,
                      device: int = 0, finish: Optional[dict] = None, adaptive: Optional[dict] = None, directional: bool = False):
        """The lightmap of `mesh` (a StaticMesh of this scene, or any objload.Mesh) in one call (mi_bake_lightmap): the RgbImage bytes
        [height, width, 3] u8 of its uv atlas, `samples` cosine-distributed gathers per texel, each from its own jittered position inside
        the texel (jitter) or all from the centre.  The atlas is rasterised, sampled and traced on the GPU: only the mesh goes up and the
        image comes back.  This scene's camera supplies path_depth, max_trace_dist and gamma; `offset` lifts the points off the surface
        along the normal.
        `finish` (None: the raw bake, as above) is a dict of lightmap_finish's parameters (levels, normal_power_log2, sigma_plane, reach,
        sigma_color, dilate; {} for the defaults): the bake's f32 image is then filtered and dilated on the GPU (mi_lightmap_finish),
        guided by the atlas's centre table (Context.lightmap_texels with rows=1, the same offset), and the call returns the finished
        lightmap (out [height, width, 3] f32, valid [height, width] bool) instead of bytes.
        A true "variance" key in `finish` selects the variance-guided finish: the bake also returns its second moments
        (mi_bake_lightmap_moments), the remaining keys are lightmap_finish_var's parameters (levels, normal_power_log2, sigma_plane,
        reach, sigma_color, color_floor, dilate), and the call returns (out, var [height, width] f32, valid) (mi_lightmap_finish_var).
        Without the key, or with a false one, nothing changes.
        `adaptive` (None: a uniform bake, as above) is a dict with round_samples, max_rounds, target_rel and target_abs, and optionally
        first_samples (default: `samples`): the bake is mi_bake_lightmap_adaptive, which gives every texel first_samples samples and
        then up to max_rounds rounds of round_samples more to the texels lightmap_select picks.  Without `finish` the call returns the
        bytes of the merged mean; with a fixed finish that is applied to the merged mean; with finish={"variance": True, ...} the
        finish takes the bake's per-texel counts (mi_lightmap_finish_var_counts).
        `directional` (False: everything above) bakes a directional lightmap (mi_bake_lightmap_sh): the call returns
        (sh [height, width, 9, 3] f32, mean [height, width, 3] f32) — the SH L2 radiance records lightmap_sh_eval turns into the
        irradiance at any normal, beside the mean the plain bake stores.  With `finish` (lightmap_finish's parameters; no "variance"
        key) both are finished on the GPU, by mi_lightmap_finish_sh and mi_lightmap_finish with the same parameters, and the call
        returns (sh, mean, valid).  It does not combine with `adaptive`."""
        from dataclasses import replace
        cam = replace(self.camera, screen_width=int(width), screen_height=int(height), aa_sample_count=int(samples))
        check_point_table(cam, np.zeros((height, width, 3), np.float32), np.zeros((height, width, 3), np.float32))
        if directional and (adaptive is not None or (finish is not None and "variance" in finish)):
            raise ValueError("a directional bake combines with neither `adaptive` nor the variance-guided finish")
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            if directional:
                sh, f32, _, _, _, _ = ctx.bake_lightmap_sh(cam, mesh, jitter=jitter, offset=offset, seed=seed, want_f32=True, want_u8=False)
                if finish is None:
                    return sh, f32
                points, normals, _ = ctx.lightmap_texels(mesh, int(width), int(height), rows=1, offset=offset, want_triangle=False)
                sh, valid = ctx.lightmap_finish_sh(sh, points, normals, **finish)
                f32, _ = ctx.lightmap_finish(f32, points, normals, **finish)
                return sh, f32, valid
            if adaptive is not None:
                ad = dict(adaptive)
                ad.setdefault("first_samples", int(samples))
                counts, m2, f32, u8, _, _, _ = ctx.bake_lightmap_adaptive(cam, mesh, jitter=jitter, offset=offset, seed=seed,
                                                                          want_f32=finish is not None, want_u8=finish is None, **ad)
                if finish is None:
                    return u8
                finish = dict(finish)
                points, normals, _ = ctx.lightmap_texels(mesh, int(width), int(height), rows=1, offset=offset, want_triangle=False)
                if finish.pop("variance", False):
                    return ctx.lightmap_finish_var_counts(f32, m2, counts, points, normals, **finish)
                return ctx.lightmap_finish(f32, points, normals, **finish)
            if finish is None:
                _, u8, _, _, _ = ctx.bake_lightmap(cam, mesh, jitter=jitter, offset=offset, seed=seed, want_f32=False, want_u8=True)
                return u8
            if "variance" in finish:
                finish = dict(finish)
                if finish.pop("variance"):
                    m2, f32, _, _, _, _ = ctx.bake_lightmap_moments(cam, mesh, jitter=jitter, offset=offset, seed=seed, want_f32=True,
                                                                    want_u8=False)
                    points, normals, _ = ctx.lightmap_texels(mesh, int(width), int(height), rows=1, offset=offset, want_triangle=False)
                    return ctx.lightmap_finish_var(f32, m2, int(samples), points, normals, **finish)
            f32, _, _, _, _ = ctx.bake_lightmap(cam, mesh, jitter=jitter, offset=offset, seed=seed, want_f32=True, want_u8=False)
            points, normals, _ = ctx.lightmap_texels(mesh, int(width), int(height), rows=1, offset=offset, want_triangle=False)
            return ctx.lightmap_finish(f32, points, normals, **finish)
        finally:
            ctx.close()

    def render_probes(self, points, seed: int = 1, device: int = 0):
        """Light probes (mi_render_probes): the radiance arriving at a table of points in free space (probe_grid makes one), projected
        onto the SH L2 basis — per probe aa_sample_count directions uniform over the sphere, drawn on the GPU, each shaded by
        Scene::shade_ray.  This scene's camera supplies the table's size (screen_width x screen_height probes), aa_sample_count,
        path_depth, max_trace_dist and gamma.  Returns (sh [H, W, 9, 3] f32, mean [H, W, 3] f32, u8 [H, W, 3], sig [H, W] u32, stats)."""
        p, _ = check_probe_table(self.camera, points)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            return ctx.render_probes(self.camera, p, seed=seed, want_sig=True)
        finally:
            ctx.close()

    def irradiance_volume(self, lo, hi, counts, samples: int, seed: int = 1, device: int = 0, valid=None) -> "ProbeVolume":
        """An irradiance volume of this scene: probe_grid(lo, hi, counts), then render_probes with `samples` directions per probe, then the
        first n records of its sh as a ProbeVolume — .sample(points, normals) lights whatever moves through the scene.  This scene's
        camera supplies path_depth and max_trace_dist.  `valid` (None, or [n]: 0 = the probe takes no part) is the caller's."""
        from dataclasses import replace
        cnt = tuple(int(c) for c in counts)
        if len(cnt) != 3 or not all(1 <= c <= PV_MAX_COUNT for c in cnt) or cnt[0] * cnt[1] * cnt[2] > PV_MAX_PROBES:
            raise ValueError(f"counts must be three integers in 1 .. {PV_MAX_COUNT} with at most 2^22 probes, got {cnt}")
        check_probe_volume(lo, hi, (1, 1, 1), np.zeros((1, 9, 3), np.float32))          # the box, before anything is rendered
        pts, n = probe_grid(lo, hi, cnt)
        cam = replace(self.camera, screen_width=pts.shape[1], screen_height=pts.shape[0], aa_sample_count=int(samples))
        p, _ = check_probe_table(cam, pts)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            sh, _, _, _, _ = ctx.render_probes(cam, p, seed=seed, want_f32=False, want_u8=False)
        finally:
            ctx.close()
        return ProbeVolume(lo, hi, tuple(int(c) for c in counts), sh.reshape(-1, 9, 3)[:n].copy(), valid)

    def shade_rays(self, origins, dirs, seed: int = 1, first_key: int = 0, device: int = 0) -> np.ndarray:
        """Scene::shade_ray (tracing.rs:300-324) at level 0 for a batch of rays, with this scene's camera settings."""
        o, d, _, _ = check_rays(origins, dirs)
        check_shade_camera(self.camera)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            return ctx.shade_rays(self.camera, o, d, seed=seed, first_key=first_key)
        finally:
            ctx.close()

    def shade_rays_baked(self, origins, dirs, lightmaps, t_min: float = 0.001, t_max: float = float("inf"), device: int = 0):
        """Baked lighting for a batch of rays: one ray query and one lightmap lookup per lit object, no path is traced.  `lightmaps` maps
        an index into Scene.objects to (sh [H, W, 9, 3], valid [H, W] or None): that object's finished directional lightmap
        (bake_lightmap(directional=True) + lightmap_finish_sh).  Returns (rgb [n, 3] f32, RayHits): shade_hits_baked of the hits of
        intersect_rays(resolve=True), the lookups on the GPU (mi_lightmap_sh_sample).  An entry may also be a Bc6hLightmap: a plain
        irradiance lightmap stored as BC6H blocks, read through mi_lightmap_sample_bc6h."""
        o, d, t_min, t_max = check_rays(origins, dirs, t_min, t_max)
        ctx = Context(device)
        try:
            ctx.upload(self.flatten())
            hits = ctx.intersect_rays(o, d, t_min, t_max, resolve=True)
            return shade_hits_baked(hits, lightmaps, ctx.lightmap_sh_sample, ctx.lightmap_sample_bc6h), hits
        finally:
            ctx.close()


def shade_hits_baked(hits: RayHits, lightmaps, sample=lightmap_sh_sample, sample_bc6h=lightmap_sample_bc6h) -> np.ndarray:
    """The baked-lighting colour [n, 3] f32 of resolved ray hits: a miss is 0; a hit on an object listed in `lightmaps`
    ({object index: (sh [H, W, 9, 3], valid or None)}) that has texture coordinates is
    emission + (albedo * E) * f32(1 / pi) with E = sample(sh, hit uv, hit normal, valid)[0] — the hit's shading normal, so a normal map
    shows; every other hit is its emission.  All f32, one rounding per operation.  `sample` is lightmap_sh_sample (the definition) or
    Context.lightmap_sh_sample.  Where an entry of `lightmaps` is a Bc6hLightmap m instead of a pair, E is the plain irradiance
    sample_bc6h(m.blocks_chain, m.width, m.height, hit uv, m.lod, m.valid_chain)[0] (lightmap_sample_bc6h or Context.lightmap_sample_bc6h)."""
    f32 = np.float32
    obj = np.asarray(hits.object)
    rgb = np.zeros((len(obj), 3), f32)
    hit = obj >= 0
    rgb[hit] = hits.material["emission"][hit]
    for index, entry in lightmaps.items():
        at = np.nonzero((obj == int(index)) & hits.has_uv)[0]
        if len(at) == 0:
            continue
        if isinstance(entry, Bc6hLightmap):
            E, _ = sample_bc6h(entry.blocks_chain, entry.width, entry.height, hits.uv[at], entry.lod, entry.valid_chain)
        else:
            sh, valid = entry
            E, _ = sample(sh, hits.uv[at], hits.normal[at], valid)
        with np.errstate(all="ignore"):
            rgb[at] = hits.material["emission"][at] + (hits.material["albedo"][at] * E) * f32(0.3183098861837907)
    assert rgb.dtype == np.float32
    return rgb
