#!/usr/bin/env python
"""Throughput of the ray queries (mi_intersect_rays_device) on one MI355X.

For cfg2 (Cornell box + teapot) and cfg4 (textured drone) at 1920x1080 two ray sets are measured, each with `resolve` on (every
output array) and off (the visibility form: object and distance only):
  camera   one ray per pixel of the frame's camera: the pinhole ray through the pixel centre (built here in numpy; a measuring tool,
           not a parity surface, so the thin lens and the jitter of Camera::generate_rays are left out)
  bounce   the first-bounce rays of those: origin = the hitpoint the library returned for the camera ray, direction = a seeded random
           unit vector (one per camera hit; the misses are dropped)
Per set: 5 warm-up calls, then --calls timed calls (default 20) through the device entry point on device-resident arrays.  Two rates
are printed per row, from the median call: Mrays/s from mi_last_kernel_ms (HIP events around the kernel) and from the wall clock around
call + synchronise.  One JSON line per row; no pass / fail bar.  Needs a GPU: there is no CPU fallback.

--mode occlusion compares the any-hit query (mi_occluded_rays_device) with the visibility form of mi_intersect_rays_device on the same
rays, in the same process and context, the two ALTERNATING call by call (5 warm-up pairs, then --calls timed pairs; median / min / max of
mi_last_kernel_ms for each).  Ray sets: `camera` and `bounce` as above, and
  shadow   origin = the library's camera hitpoint, direction = the unit vector towards the fixed point (0, 5.9, 0) just under the ceiling
           light, per-ray ray_t_max = the distance to that point - 1e-3.  The visibility form has one scalar interval per call and would
           need one call per distinct distance (about as many as rays), so it runs ONCE with t_max = +inf.  A longer interval can only
           add box and triangle work to a closest-hit walk, so on this row the comparison is generous to the any-hit query, and the two
           do not answer the same question; the visibility row says so ("t_max": "inf (scalar)").

--mode render compares ray-table rendering (mi_render_rays_device: the wavefront pipeline fed from a table) with mi_shade_rays_device (the
recursive kernel) on the same rays: one table per scene built from the `camera` rays above, rays_per_pixel = 1.  In one context: the
shade query on the table's rays, then the table render with aa_sample_count = 1 and with 16; for each 5 warm-up calls, then --calls
timed calls, median / min / max of mi_last_kernel_ms and Msamples/s (rays x aa_sample_count) from the median.  Context for users, not
a pass bar.

--mode hemisphere compares hemisphere occlusion (mi_hemisphere_occlusion_device: the rays are made on the GPU and reduced per point)
with mi_occluded_rays_device fed the IDENTICAL rays, pre-made and already resident — so that run excludes what the feature saves, making
and uploading the rays.  Points and normals: the library's camera hits (zero normals dropped), at most --points of them, evenly
strided; 64 samples per point; t_max = 4 in units of |d| (|d| <= 1: about 3 world units in a 6 x 5 x 6 box), flags 0.  The pre-made
directions come from the library itself: 64 calls with n_samples = 1, first_sample = s and the EMPTY interval [1, 0], under which
every sample is open and out_bent is that one direction; ray i * 64 + s of the any-hit call is sample s of point i, so a wave holds
one point's 64 samples in both kernels.  The two alternate call by call (5 warm-up pairs, then --calls timed pairs; median / min / max
of mi_last_kernel_ms) and the tool checks that the any-hit answers reduce to the hemisphere counts.

--mode bake compares point-table rendering (mi_render_points_device: the camera pass draws each sample's hemisphere direction itself)
with ray-table rendering (mi_render_rays_device) fed the IDENTICAL rays, pre-made and already resident — so that run excludes what the
feature saves, making and uploading aa_sample_count directions per texel.  The point table is one [H][W] row: the library's camera
first hits, point = hitpoint + 1e-3 * normal; misses (and hits with a zero normal) are empty texels, whose share is printed.
aa_sample_count = 16, path_depth 10.  The pre-made directions are restated on the host in numpy (hemisphere_dirs below: the stream
(seed, W*H + y*W + x, s), rand_sphere_vec, |y|, the rotation from unit y, operation for operation in f32); an empty texel's ray in the
table starts far outside the scene and meets nothing.  The two alternate call by call (5 warm-up pairs, then --calls timed pairs;
median / min / max of mi_last_kernel_ms, and their ratio) and the tool checks that the two compact images agree bit for bit on the live
texels: if they did not, the restated directions would not be the kernel's and the rows would not compare like with like.

--mode probes compares light-probe rendering (mi_render_probes_device: the camera pass draws each sample's full-sphere direction, and
wf_reduce_sh projects the samples onto the SH L2 basis) with ray-table rendering (mi_render_rays_device) fed the IDENTICAL rays,
pre-made and resident — the same protocol as --mode bake, and the same exclusion: the ray-table run neither makes nor uploads its
directions, and it produces no SH output at all, so the rows are like for like in the traced paths only.  The probes are a cubic grid
inside the Cornell box (probe_grid over [-2.8, 2.8] x [0.2, 5.8] x [-2.8, 2.8]) laid out as a square table: 4096 probes x 256 samples
(a 64 x 64 table) and 65536 probes x 64 samples (256 x 256), path_depth 10.  The pre-made directions are rand_sphere_vec restated in
numpy (sphere_dirs below).  Each row reports median / min / max of mi_last_kernel_ms; the probes row also the time of wf_reduce_sh
(entry 7 of mi_last_pipeline_ms: HIP events around its launches) and its share of the kernel time.  The tool checks that the two
compact images agree bit for bit.

--mode atlas times the lightmap atlas (mi_lightmap_texels_device / mi_bake_lightmap) against the host helper lightmap_texels on the drone
of config 4, at --atlas-sizes (square atlases, default 1024 and 2048), aa_sample_count = 16, path_depth 10.  Per size: the helper's wall
time (one run: it takes seconds); the kernels' time (HIP events around count, scan, fill and resolve: mi_last_kernel_ms) with the mesh
resident, rows = 1 and rows = 16 jittered, 5 warm-up calls then --calls timed ones; and the whole bake both ways, wall clock around the
blocking calls, --atlas-bakes times each, alternating: mi_bake_lightmap (mesh up, table made on the GPU, render, image down) against
lightmap_texels + mi_render_points (table made on the host, uploaded, the same render).  The tool checks that the GPU's triangle plane
equals the helper's and that the two bakes give the same bytes.  --atlas-grid N replaces the drone (1736 triangles in this repository's
asset) by a height field of N x N quads, 2 N^2 triangles, for the table's timings alone.

--mode finish times lightmap finishing (mi_lightmap_finish_device) on the drone's atlas at --finish-sizes (square, default 1024, 2048 and
4096) with levels = 5 and dilate = 8, on device-resident tables: the guides are mi_lightmap_texels_device's centre table, the image is
seeded noise on the covered texels (the passes' cost does not depend on the colours).  A call's kernels are timed by HIP events
(mi_last_kernel_ms: their sum), 5 warm-up calls then --calls timed ones, medians; one pass's time is the difference between the medians of
two calls that differ by that pass (levels = k + 1 against levels = k, both without dilation; levels = 5 with dilate = 8 against
dilate = 0, divided by 8).  Every level is run in both forms of lmf_atrous, in two contexts created under the developer knob
MI_RT_LMF_LDS_MAX_STEP (0: every step reads HBM directly; 8: steps 1 .. 8 stage tile and halo in LDS; step 16 has no LDS form), the whole
call also in a context with the library's own threshold, and the images of all three are compared bit for bit.  Per level: effective GB/s on the compulsory bytes (60 B per texel: 36 B of guides and 12 B of
colour read, 12 B written), beside the rate of a device-to-device copy that moves the same byte count, timed by events in the same run.

--mode volume times irradiance-volume sampling (mi_probe_volume_sample_device) on device-resident tables: volumes of --volume-grids probes
per axis (default 16 and 32) over the bounding box of the drone's atlas, seeded sh (the cost does not depend on the values), every fifth
probe invalid, MI_PV_NORMAL_WEIGHT set; --volume-points (default 2^20 and 2^22) surface points taken from the covered texels of the
drone's 4096 x 4096 atlas table in raster order ("coherent": neighbouring lanes share corners) and the same points shuffled
("incoherent").  A call's two kernels are timed by HIP events (mi_last_kernel_ms), 5 warm-up calls then --calls timed ones: median and
min - max.  pv_prepare alone is a call with one point.  The floor is a device-to-device copy of the same input and output bytes (40 B per
point: 24 in, 16 out), timed by events in the same run.  The first 4096 points of every row are compared with the helper bit for bit.

--mode variance times the lightmap variance calls on device-resident tables, HIP events, 5 warm-up and --calls timed calls, median and
min - max.  Moments: on the drone's atlas at 1024 x 1024 (mi_lightmap_texels_device's centre table), aa_sample_count = 16, path_depth 10,
mi_render_points_moments_device alternates call by call with mi_render_points_device; the rows give mi_last_kernel_ms of each, the ratio
of the medians, and wf_reduce_m2 (entry 7 of mi_last_pipeline_ms) beside wf_reduce (entry 2) of the same runs, which read the same
sample slots.  The tool checks that the two compact images agree bit for bit.  Finish: at --finish-sizes, levels = 5 and dilate = 8,
mi_lightmap_finish_var_device (sigma_color 8, color_floor 1e-6) alternates with mi_lightmap_finish_device (sigma_color 8) on seeded noise
over the covered texels, the moments those of 16 samples with a relative standard deviation of 0.3; the rows give each call's time and
the ratio (three kernels per level instead of one).

--mode directional times the directional lightmap calls (mi_render_points_sh_device, mi_lightmap_finish_sh_device,
mi_lightmap_sh_eval_device); its protocol and the measured figures are in directional_rows' docstring.

--mode lookup times the lightmap lookup kernels (mi_lightmap_sample_device at 3 and 27 channels, mi_lightmap_sh_sample_device) at
--lookup-sizes and --volume-points; its protocol is in lookup_rows' docstring, the measured figures in DESIGN.md.

--mode mips times the lightmap mip chain (mi_lightmap_mips_device, five levels per launch against one) and the trilinear lookups
(mi_lightmap_sample_lod_device, mi_lightmap_sh_sample_lod_device) at --lookup-sizes and --volume-points; its protocol is in mips_rows'
docstring, the measured figures in DESIGN.md."""
import argparse
import json
import os
import sys
import time

import torch  # first HIP runtime in the process (see cs397raytracingsp22_amd/abi.py)
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from cs397raytracingsp22_amd import Context, abi, scenes  # noqa: E402


# --mode packed (appended to the notes above): times mi_lightmap_pack_device / mi_lightmap_unpack_device against a device copy of the same
# bytes, and every packed lookup against its f32 twin on coherent and shuffled uv, with and without lod (packed_rows' docstring).
# --mode bc6h (appended to the notes above): times mi_lightmap_bc6h_encode_device (rounds 0 and 2) and mi_lightmap_bc6h_decode_device against a
# device copy of the f32 bytes and against lmp_pack RGB9E5, the BC6H lookup against the f32 and RGB9E5 lookups of the same chain, and reports
# the relative RMSE of BC6H, RGB9E5 and f16 on a finished cube bake (bc6h_rows' docstring).
# --mode adaptive (appended to the notes above): times mi_bake_lightmap_adaptive (16 first samples, 2 rounds of 16, the relative target the
# median of round 0's error over its luminance) on the cube in the one-light box and on the drone, atlas --atlas-sizes[0] squared, against
# uniform mi_bake_lightmap_moments bakes at the adaptive run's own slots per texel and at first + max_rounds * round_samples; reports every
# bake's mean absolute and mean relative error over the covered texels against a uniform bake at 16 x the larger count with another seed, and the HIP-event
# times of select, gather and merge on resident tables beside the kernel time of the round's render.  --atlas-bakes timed bakes per row.
def pinhole_rays(cam):
    """Rays through the pixel centres of `cam` (tracing.rs:160-163,187-191 without jitter and lens), row-major."""
    W, H = cam.screen_width, cam.screen_height
    eye, view, up = (np.asarray(v, np.float64) for v in (cam.eyepoint, cam.view_dir, cam.up))
    right = np.cross(view, up)
    right /= np.linalg.norm(right)
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    cx, cy = (x + 0.5 - 0.5 * W) / H, (0.5 * H - y - 0.5) / H
    d = cx[..., None] * right + cy[..., None] * up + cam.focal_length * view
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    o = np.broadcast_to(eye, d.shape)
    return np.ascontiguousarray(o.reshape(-1, 3), np.float32), np.ascontiguousarray(d.reshape(-1, 3), np.float32)


def measure(ctx, o, d, t_max, resolve, calls, warmup):
    dev = torch.device("cuda:0")
    n = len(o)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_obj, t_t = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    extra = [None] * 5
    keep = []
    if resolve:
        keep = [torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev),
                torch.empty(n, dtype=torch.int32, device=dev), torch.empty((n, 2), dtype=torch.float32, device=dev),
                torch.empty((n, 10), dtype=torch.int32, device=dev)]
        extra = [t.data_ptr() for t in keep]
    torch.cuda.synchronize()
    kernel_ms, wall_ms = [], []
    for k in range(warmup + calls):
        t0 = time.perf_counter()
        ctx.intersect_rays_device(n, t_o.data_ptr(), t_d.data_ptr(), t_obj.data_ptr(), t_t.data_ptr(), *extra, t_min=0.001, t_max=t_max, seed=1)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= warmup:
            kernel_ms.append(ctx.last_kernel_ms())
            wall_ms.append((t1 - t0) * 1e3)
    hits = int((t_obj >= 0).sum().item())
    return float(np.median(kernel_ms)), float(np.median(wall_ms)), float(np.min(kernel_ms)), float(np.max(kernel_ms)), hits


def measure_pair(ctx, o, d, t_max, ray_t_max, calls, warmup):
    """The any-hit query and the visibility form on the same device-resident rays, alternating.  Returns two dicts of kernel times."""
    dev = torch.device("cuda:0")
    n = len(o)
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_tm = torch.from_numpy(ray_t_max).to(dev) if ray_t_max is not None else None
    t_occ = torch.empty(n, dtype=torch.uint8, device=dev)
    t_obj, t_t = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
    vis_t_max = float("inf") if ray_t_max is not None else t_max
    torch.cuda.synchronize()
    occ_ms, vis_ms = [], []
    for k in range(warmup + calls):
        ctx.occluded_rays_device(n, t_o.data_ptr(), t_d.data_ptr(), t_occ.data_ptr(), t_tm.data_ptr() if t_tm is not None else None,
                                 t_min=0.001, t_max=t_max, seed=1)
        torch.cuda.synchronize()
        a = ctx.last_kernel_ms()
        ctx.intersect_rays_device(n, t_o.data_ptr(), t_d.data_ptr(), t_obj.data_ptr(), t_t.data_ptr(), t_min=0.001, t_max=vis_t_max, seed=1)
        torch.cuda.synchronize()
        b = ctx.last_kernel_ms()
        if k >= warmup:
            occ_ms.append(a)
            vis_ms.append(b)
    stat = lambda v: {"kernel_ms_median": round(float(np.median(v)), 4), "kernel_ms_min": round(float(np.min(v)), 4),
                      "kernel_ms_max": round(float(np.max(v)), 4), "mrays_per_s_kernel": round(n / float(np.median(v)) / 1e3, 1)}
    occ = dict(stat(occ_ms), query="occluded", true=int((t_occ != 0).sum().item()),
               t_max="per ray" if ray_t_max is not None else t_max)
    vis = dict(stat(vis_ms), query="visibility", true=int((t_obj >= 0).sum().item()),
               t_max="inf (scalar)" if ray_t_max is not None else t_max)
    return occ, vis


HEMI_SAMPLES = 64
HEMI_T_MAX = 4.0


def hemisphere_rows(ctx, cfg, points, normals, calls, warmup):
    dev = torch.device("cuda:0")
    n, S = len(points), HEMI_SAMPLES
    t_p, t_n = torch.from_numpy(points).to(dev), torch.from_numpy(normals).to(dev)
    t_open = torch.empty(n, dtype=torch.int32, device=dev)
    t_bent = torch.empty((n, 3), dtype=torch.float32, device=dev)
    t_d = torch.empty((n, S, 3), dtype=torch.float32, device=dev)
    for s in range(S):                                   # the directions, from the library: one sample, the empty interval
        ctx.hemisphere_occlusion_device(n, t_p.data_ptr(), t_n.data_ptr(), t_open.data_ptr(), 1, d_bent=t_bent.data_ptr(),
                                        t_min=1.0, t_max=0.0, seed=1, first_key=0, first_sample=s)
        torch.cuda.synchronize()
        if not bool((t_open == 1).all().item()):
            raise SystemExit("ray_query_bench: a sample is occluded under the empty interval; the directions cannot be read back")
        t_d[:, s, :] = t_bent
    t_o = t_p[:, None, :].expand(n, S, 3).contiguous()
    t_occ = torch.empty(n * S, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    hemi_ms, occ_ms = [], []
    for k in range(warmup + calls):
        ctx.hemisphere_occlusion_device(n, t_p.data_ptr(), t_n.data_ptr(), t_open.data_ptr(), S, d_bent=t_bent.data_ptr(),
                                        t_min=0.001, t_max=HEMI_T_MAX, seed=1, first_key=0)
        torch.cuda.synchronize()
        a = ctx.last_kernel_ms()
        ctx.occluded_rays_device(n * S, t_o.data_ptr(), t_d.data_ptr(), t_occ.data_ptr(), None, t_min=0.001, t_max=HEMI_T_MAX, seed=1)
        torch.cuda.synchronize()
        b = ctx.last_kernel_ms()
        if k >= warmup:
            hemi_ms.append(a)
            occ_ms.append(b)
    reduced = (t_occ.view(n, S) == 0).sum(dim=1).to(torch.int32)
    mismatches = int((reduced != t_open).sum().item())
    stat = lambda v: {"kernel_ms_median": round(float(np.median(v)), 4), "kernel_ms_min": round(float(np.min(v)), 4),
                      "kernel_ms_max": round(float(np.max(v)), 4), "mrays_per_s_kernel": round(n * S / float(np.median(v)) / 1e3, 1)}
    base = {"config": cfg, "mode": "hemisphere", "n_points": n, "n_samples": S, "t_max": HEMI_T_MAX, "calls": calls,
            "open_share": round(float(t_open.sum().item()) / (n * S), 4), "count_mismatches": mismatches}
    rows = [dict(base, query="hemisphere_occlusion", **stat(hemi_ms)), dict(base, query="occluded_rays (pre-made rays)", **stat(occ_ms)),
            dict(base, query="ratio hemisphere / occluded", kernel_ms_median=round(float(np.median(hemi_ms)) / float(np.median(occ_ms)), 4))]
    for row in rows:
        print(json.dumps(row), flush=True)
    if mismatches:
        raise SystemExit(f"ray_query_bench: {mismatches} points whose any-hit answers do not reduce to the hemisphere count")
    return rows


BAKE_AA = 16


def _lowbias32(x):
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _rotl(x, k):
    return (x << np.uint32(k)) | (x >> np.uint32(32 - k))


def _ulps_eq(a, b):
    """approx::ulps_eq!(a, b) with f32 defaults (epsilon = f32::EPSILON, max_ulps = 4), b a scalar"""
    b = np.float32(b)
    near = np.abs(a - b) <= np.float32(1.1920929e-07)
    ia, ib = a.view(np.int32).astype(np.int64), int(np.array(b).view(np.int32))
    return near | (((a < 0) == (b < 0)) & (np.abs(ia - ib) <= 4))


def sphere_dirs(n, seed, key0, sample):
    """rand_sphere_vec as mi_render_points / mi_render_probes draw it on the direction stream, for pixels i = 0 .. n-1 with keys key0 + i
    and one sample index: [n, 3] f32 points of the unit ball.  Every step is the kernel's f32 / u32 operation, in its order."""
    F, U = np.float32, np.uint32
    with np.errstate(over="ignore"):
        seed_key = _lowbias32(np.array([seed], U) ^ U(0x68e31da4))[0]
        p0 = _lowbias32(np.arange(n, dtype=U) + U(key0) + seed_key)
        p1 = _lowbias32(p0 ^ U(0xb5297a4d))
        smp = np.array([sample], U)
        s0 = _lowbias32(p0 + (smp * U(0x9e3779b9))[0])
        s1 = _lowbias32(p1 ^ (smp * U(0x85ebca6b))[0])
        s1 = np.where((s0 | s1) == 0, U(1), s1)

        def genm11():                                   # xoroshiro64**, then gen_range(-1.0..1.0): value1_2 * 2 + (-1 - 2)
            nonlocal s0, s1
            res = _rotl(s0 * U(0x9e3779bb), 5) * U(5)
            t = s1 ^ s0
            s0, s1 = _rotl(s0, 26) ^ t ^ (t << U(9)), _rotl(t, 13)
            return (U(0x3f800000) | (res >> U(9))).view(F) * F(2.0) + F(-3.0)

        v = np.zeros((n, 3), F)
        todo = np.ones(n, bool)
        while todo.any():                               # rand_sphere_vec: draw until the point lies in the unit ball
            c = np.stack([genm11(), genm11(), genm11()], axis=-1)       # (lanes that are done draw on; their stream is not used again)
            ok = todo & (((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]) <= F(1.0))
            v[ok] = c[ok]
            todo &= ~ok
    return v


def hemisphere_dirs(normals, seed, key0, sample):
    """sample_hemisphere(normal) as mi_render_points draws it, for texels i = 0 .. n-1 with keys key0 + i and one sample index:
    normals [n, 3] f32 (non-zero, finite) -> directions [n, 3] f32.  Every step is the kernel's f32 / u32 operation, in its order."""
    F = np.float32
    v = sphere_dirs(len(normals), seed, key0, sample)
    v[:, 1] = np.abs(v[:, 1])
    nx, ny, nz = (np.ascontiguousarray(normals[:, k], F) for k in range(3))
    ident = _ulps_eq(ny, 1.0)
    with np.errstate(all="ignore"):
        k = np.sqrt(F(1.0) * ((nx * nx + ny * ny) + nz * nz))
        flip = _ulps_eq(ny / k, -1.0)
        s = k + ny
        cx, cz = nz, -nx
        inv = F(1.0) / np.sqrt(s * s + ((cx * cx + F(0.0)) + cz * cz))
        qs, qx, qz = np.where(flip, F(0.0), s * inv), np.where(flip, F(0.0), cx * inv), np.where(flip, F(-1.0), cz * inv)
    x2, z2 = qx + qx, qz + qz
    xx2, xz2, zz2, sz2, sx2 = x2 * qx, x2 * qz, z2 * qz, z2 * qs, x2 * qs
    c0 = (F(1.0) - zz2, sz2, xz2)
    c1 = (-sz2, (F(1.0) - xx2) - zz2, sx2)
    c2 = (xz2, -sx2, F(1.0) - xx2)
    d = np.stack([(c0[a] * v[:, 0] + c1[a] * v[:, 1]) + c2[a] * v[:, 2] for a in range(3)], axis=-1).astype(F)
    d[ident] = v[ident]
    return d


def bake_rows(ctx, cfg, sc, first, calls, warmup):
    from cs397raytracingsp22_amd import dist as pdist
    dev = torch.device("cuda:0")
    cam = sc.camera
    W, H = cam.screen_width, cam.screen_height
    cam.aa_sample_count = BAKE_AA
    live = (first.object >= 0) & np.any(first.normal != 0.0, axis=1)
    nrm = np.where(live[:, None], first.normal, np.float32(0.0)).astype(np.float32)
    pts = np.where(live[:, None], first.hitpoint + np.float32(1e-3) * first.normal, np.float32(0.0)).astype(np.float32)
    idx = np.flatnonzero(live)
    t_p, t_n = torch.from_numpy(pts).to(dev), torch.from_numpy(nrm).to(dev)        # [H*W, 3] row-major = a table [1][H][W][3]
    # the same rays as a ray table [aa][H][W][3]; an empty texel's ray starts far above the scene, points away and meets nothing
    o_row = pts.copy()
    o_row[~live] = (0.0, 1.0e6, 0.0)
    t_o = torch.from_numpy(o_row).to(dev)[None].expand(BAKE_AA, W * H, 3).contiguous()
    t_d = torch.empty((BAKE_AA, W * H, 3), dtype=torch.float32, device=dev)
    for s in range(BAKE_AA):
        row = np.zeros((W * H, 3), np.float32)
        row[:, 1] = 1.0
        keyed = np.zeros((W * H, 3), np.float32)
        keyed[:, 1] = 1.0                                # (a unit normal for the empty texels: their directions are discarded)
        keyed[idx] = nrm[idx]
        row[idx] = hemisphere_dirs(keyed, 1, W * H, s)[idx]
        t_d[s] = torch.from_numpy(row).to(dev)
    n_compact = pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS
    c_pts = torch.empty((n_compact, 3), dtype=torch.float32, device=dev)
    c_rays = torch.empty((n_compact, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    pts_ms, rays_ms = [], []
    for k in range(warmup + calls):
        ctx.render_points_device(cam, t_p.data_ptr(), t_n.data_ptr(), 1, c_pts.data_ptr(), seed=1)
        torch.cuda.synchronize()
        a = ctx.last_kernel_ms()
        seg_p = ctx.last_pipeline_counts()["segments"]
        ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), BAKE_AA, c_rays.data_ptr(), seed=1)
        torch.cuda.synchronize()
        b = ctx.last_kernel_ms()
        seg_r = ctx.last_pipeline_counts()["segments"]
        if k >= warmup:
            pts_ms.append(a)
            rays_ms.append(b)
    # compare on the live texels, through the image layout
    img_p = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    img_r = torch.empty((H, W, 3), dtype=torch.float32, device=dev)
    ctx.unpermute_device(cam, 1, c_pts.data_ptr(), img_p.data_ptr())
    ctx.unpermute_device(cam, 1, c_rays.data_ptr(), img_r.data_ptr())
    torch.cuda.synchronize()
    t_live = torch.from_numpy(live.reshape(H, W)).to(dev)
    differ = int(((img_p.view(torch.int32) != img_r.view(torch.int32)).any(dim=-1) & t_live).sum().item())
    n_live = int(live.sum())
    stat = lambda v: {"kernel_ms_median": round(float(np.median(v)), 4), "kernel_ms_min": round(float(np.min(v)), 4),
                      "kernel_ms_max": round(float(np.max(v)), 4),
                      "msamples_per_s_kernel": round(n_live * BAKE_AA / float(np.median(v)) / 1e3, 1)}
    ratios = [a / b for a, b in zip(pts_ms, rays_ms)]
    base = {"config": cfg, "mode": "bake", "width": W, "height": H, "aa_sample_count": BAKE_AA, "path_depth": cam.path_depth,
            "calls": calls, "live_texels": n_live, "empty_share": round(1.0 - n_live / (W * H), 4), "live_texels_that_differ": differ}
    rows = [dict(base, query="render_points", segments=seg_p, mean_radiance=round(float(img_p.mean().item()), 6), **stat(pts_ms)),
            dict(base, query="render_rays (pre-made rays)", segments=seg_r, mean_radiance=round(float(img_r.mean().item()), 6),
                 **stat(rays_ms)),
            dict(base, query="ratio render_points / render_rays", kernel_ms_median=round(float(np.median(pts_ms)) / float(np.median(rays_ms)), 4),
                 pairwise_ratio_median=round(float(np.median(ratios)), 4), pairwise_ratio_min=round(float(np.min(ratios)), 4),
                 pairwise_ratio_max=round(float(np.max(ratios)), 4))]
    for row in rows:
        print(json.dumps(row), flush=True)
    if differ:
        raise SystemExit(f"ray_query_bench: {differ} live texels differ between the point-table and the ray-table render: the restated "
                         "directions are not the kernel's")
    return rows


def probes_rows(ctx, cfg, sc, calls, warmup):
    from cs397raytracingsp22_amd import dist as pdist, probe_grid
    dev = torch.device("cuda:0")
    cam = sc.camera
    rows = []
    for side, aa in ((64, 256), (256, 64)):
        cells = {64: (16, 16, 16), 256: (64, 32, 32)}[side]                  # 4096 and 65536 probes
        pts, n = probe_grid((-2.8, 0.2, -2.8), (2.8, 5.8, 2.8), cells, width=side)
        assert n == side * side and pts.shape == (side, side, 3)
        W = H = side
        cam.screen_width, cam.screen_height, cam.aa_sample_count = W, H, aa
        t_p = torch.from_numpy(pts).to(dev)                                  # [1][H][W][3]
        t_o = t_p[None].expand(aa, H, W, 3).contiguous()
        t_d = torch.empty((aa, H * W, 3), dtype=torch.float32, device=dev)
        for s in range(aa):
            t_d[s] = torch.from_numpy(sphere_dirs(W * H, 1, W * H, s)).to(dev)
        n_compact = pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS
        c_prb = torch.empty((n_compact, 3), dtype=torch.float32, device=dev)
        c_rays = torch.empty((n_compact, 3), dtype=torch.float32, device=dev)
        c_sh = torch.empty((n_compact, 27), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        prb_ms, rays_ms, sh_ms = [], [], []
        for k in range(warmup + calls):
            ctx.render_probes_device(cam, t_p.data_ptr(), 1, c_sh.data_ptr(), c_prb.data_ptr(), seed=1)
            torch.cuda.synchronize()
            a, sh = ctx.last_kernel_ms(), ctx.last_reduce_sh_ms()
            seg_p = ctx.last_pipeline_counts()["segments"]
            ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), aa, c_rays.data_ptr(), seed=1)
            torch.cuda.synchronize()
            b = ctx.last_kernel_ms()
            seg_r = ctx.last_pipeline_counts()["segments"]
            if k >= warmup:
                prb_ms.append(a)
                rays_ms.append(b)
                sh_ms.append(sh)
        differ = int((c_prb.view(torch.int32) != c_rays.view(torch.int32)).any(dim=-1).sum().item())
        stat = lambda v: {"kernel_ms_median": round(float(np.median(v)), 4), "kernel_ms_min": round(float(np.min(v)), 4),
                          "kernel_ms_max": round(float(np.max(v)), 4),
                          "msamples_per_s_kernel": round(W * H * aa / float(np.median(v)) / 1e3, 1)}
        ratios = [a / b for a, b in zip(prb_ms, rays_ms)]
        base = {"config": cfg, "mode": "probes", "probes": W * H, "aa_sample_count": aa, "path_depth": cam.path_depth, "calls": calls,
                "probes_that_differ": differ}
        out = [dict(base, query="render_probes", segments=seg_p, wf_reduce_sh_ms_median=round(float(np.median(sh_ms)), 4),
                    wf_reduce_sh_ms_min=round(float(np.min(sh_ms)), 4), wf_reduce_sh_ms_max=round(float(np.max(sh_ms)), 4),
                    wf_reduce_sh_share=round(float(np.median(sh_ms)) / float(np.median(prb_ms)), 4),
                    sh_abs_mean=round(float(c_sh.abs().mean().item()), 6), **stat(prb_ms)),
               dict(base, query="render_rays (pre-made rays)", segments=seg_r, **stat(rays_ms)),
               dict(base, query="ratio render_probes / render_rays", kernel_ms_median=round(float(np.median(prb_ms)) / float(np.median(rays_ms)), 4),
                    pairwise_ratio_median=round(float(np.median(ratios)), 4), pairwise_ratio_min=round(float(np.min(ratios)), 4),
                    pairwise_ratio_max=round(float(np.max(ratios)), 4))]
        for row in out:
            print(json.dumps(row), flush=True)
        rows += out
        if differ:
            raise SystemExit(f"ray_query_bench: {differ} probes differ between the probe and the ray-table render: the restated "
                             "directions are not the kernel's")
    return rows


SHADOW_POINT = (0.0, 5.9, 0.0)          # just under the Cornell box's ceiling light (y = 6)


def grid_mesh(n):
    """A height field of n x n quads (2 n^2 triangles) whose uv atlas is the unit square less a 1 % margin: a mesh of any size for the
    atlas timings, with analytic normals."""
    from cs397raytracingsp22_amd import cgmath, objload
    from cs397raytracingsp22_amd.geometry import StaticMesh
    g = np.linspace(0.01, 0.99, n + 1)
    u, v = np.meshgrid(g, g)
    P = np.stack([4 * u - 2, 0.3 * np.sin(7 * u) * np.cos(5 * v), 4 * v - 2], axis=-1)
    N = np.stack([-0.3 * 7 * np.cos(7 * u) * np.cos(5 * v) / 4, np.ones_like(u), 0.3 * 5 * np.sin(7 * u) * np.sin(5 * v) / 4], axis=-1)
    N /= np.linalg.norm(N, axis=-1, keepdims=True)
    k = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).reshape(-1)
    I = np.concatenate([np.stack([k, k + 1, k + n + 2], axis=1), np.stack([k, k + n + 2, k + n + 1], axis=1)])
    mesh = objload.Mesh(P.reshape(-1, 3), N.reshape(-1, 3), np.stack([u, v], axis=-1).reshape(-1, 2), I)
    return StaticMesh(mesh, None, [None] * 5, cgmath.identity())


def atlas_rows(ctx, size, calls, warmup, bakes, grid=0):
    from cs397raytracingsp22_amd import lightmap_texels
    dev = torch.device("cuda:0")
    offset = float(np.float32(1e-3))
    if grid:                                          # the table alone (it needs no scene): timings and the check against the helper
        drone, name, bakes = grid_mesh(grid), f"grid {grid}x{grid}", 0
    else:
        sc = scenes.config4(size, size, BAKE_AA, 10)
        cam = sc.camera
        drone, name = sc.objects[-1], "drone"
        ctx.upload(sc.flatten())
    mesh = drone.mesh
    t0 = time.perf_counter()
    h_p, h_n, h_cov, h_tri = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, size, size,
                                             transform=drone.transform, offset=offset, with_triangle=True)
    helper_s = time.perf_counter() - t0
    base = {"mode": "atlas", "mesh": name, "triangles": mesh.n_triangles, "vertices": mesh.n_vertices, "width": size, "height": size}
    rows = [dict(base, query="lightmap_texels (host, numpy)", wall_s=round(helper_s, 3), covered_share=round(float(h_cov.mean()), 4))]
    print(json.dumps(rows[-1]), flush=True)
    t_mesh = [torch.from_numpy(np.array(a)).to(dev) for a in (mesh.positions, mesh.normals, mesh.texcoords, mesh.indices.view(np.int32))]
    for n_rows, jitter in ((1, False), (BAKE_AA, True)):
        o_p = torch.empty((n_rows, size, size, 3), dtype=torch.float32, device=dev)
        o_n = torch.empty((n_rows, size, size, 3), dtype=torch.float32, device=dev)
        o_t = torch.empty((n_rows, size, size), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        ms = []
        for k in range(warmup + calls):
            ctx.lightmap_texels_device(t_mesh[0].data_ptr(), t_mesh[1].data_ptr(), t_mesh[2].data_ptr(), t_mesh[3].data_ptr(), mesh.n_vertices,
                                       mesh.n_triangles, size, size, o_p.data_ptr(), o_n.data_ptr(), o_t.data_ptr(), rows=n_rows, jitter=jitter,
                                       seed=1, offset=offset, transform=drone.transform)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(ctx.last_kernel_ms())
        row = dict(base, query=f"mi_lightmap_texels_device rows={n_rows}" + (" jittered" if jitter else ""), calls=calls,
                   kernel_ms_median=round(float(np.median(ms)), 4), kernel_ms_min=round(float(np.min(ms)), 4),
                   kernel_ms_max=round(float(np.max(ms)), 4), msamples_per_s_kernel=round(n_rows * size * size / float(np.median(ms)) / 1e3, 1))
        if not jitter:
            differ = int((o_t[0].cpu().numpy() != h_tri).sum())
            row["samples_whose_triangle_differs_from_the_helper"] = differ
            if differ:
                raise SystemExit(f"ray_query_bench: {differ} texels are won by another triangle than in lightmap_texels")
        rows.append(row)
        print(json.dumps(row), flush=True)
        del o_p, o_n, o_t
    if not bakes:
        return rows
    gpu_s, host_s, table_s = [], [], []
    for k in range(1 + bakes):
        t0 = time.perf_counter()
        g32, g8, _, _, _ = ctx.bake_lightmap(cam, drone, jitter=False, offset=offset, seed=1)
        t1 = time.perf_counter()
        p, n, _ = lightmap_texels(mesh.positions, mesh.normals, mesh.texcoords, mesh.indices, size, size, transform=drone.transform, offset=offset)
        t2 = time.perf_counter()
        r32, r8, _, _ = ctx.render_points(cam, p, n, seed=1)
        t3 = time.perf_counter()
        if k >= 1:
            gpu_s.append(t1 - t0)
            table_s.append(t2 - t1)
            host_s.append(t3 - t1)
    # the helper's table and the GPU's agree to 1 ulp, not to the bit, so the two images are compared by their means and their differing texels
    differ = int((g8 != r8).any(axis=-1).sum())
    rows.append(dict(base, query="mi_bake_lightmap", aa_sample_count=BAKE_AA, bakes=bakes, wall_s_median=round(float(np.median(gpu_s)), 4),
                     wall_s_min=round(float(np.min(gpu_s)), 4), wall_s_max=round(float(np.max(gpu_s)), 4),
                     mean_radiance=round(float(g32.mean()), 6)))
    rows.append(dict(base, query="lightmap_texels + mi_render_points", aa_sample_count=BAKE_AA, bakes=bakes,
                     wall_s_median=round(float(np.median(host_s)), 4), wall_s_min=round(float(np.min(host_s)), 4),
                     wall_s_max=round(float(np.max(host_s)), 4), of_which_lightmap_texels_s_median=round(float(np.median(table_s)), 4),
                     mean_radiance=round(float(r32.mean()), 6), texels_whose_u8_differs=differ))
    for row in rows[-2:]:
        print(json.dumps(row), flush=True)
    return rows


FINISH_LEVELS, FINISH_DILATE = 5, 8


def finish_rows(size, calls, warmup):
    """--mode finish at one atlas size; contexts of its own (the knob is read when a context is created)"""
    dev = torch.device("cuda:0")
    sc = scenes.config4(size, size, 1, 10)
    drone = sc.objects[-1]
    mesh = drone.mesh
    n = size * size
    t_mesh = [torch.from_numpy(np.array(a)).to(dev) for a in (mesh.positions, mesh.normals, mesh.texcoords, mesh.indices.view(np.int32))]
    pts = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
    out = {form: torch.empty((size, size, 3), dtype=torch.float32, device=dev) for form in ("direct", "lds", "default")}
    valid = torch.empty((size, size), dtype=torch.uint8, device=dev)
    ctxs = {}
    for form, knob in (("direct", "0"), ("lds", "8")):
        os.environ["MI_RT_LMF_LDS_MAX_STEP"] = knob
        ctxs[form] = Context(0)
    del os.environ["MI_RT_LMF_LDS_MAX_STEP"]
    ctxs["default"] = Context(0)                     # the library's own threshold
    ctxs["lds"].lightmap_texels_device(t_mesh[0].data_ptr(), t_mesh[1].data_ptr(), t_mesh[2].data_ptr(), t_mesh[3].data_ptr(), mesh.n_vertices,
                                       mesh.n_triangles, size, size, pts.data_ptr(), nrm.data_ptr(), None, rows=1, jitter=False, seed=1,
                                       offset=float(np.float32(1e-3)), transform=drone.transform)
    torch.cuda.synchronize()
    covered = (nrm != 0).any(dim=-1)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    img = (1.0 + 0.5 * torch.randn((size, size, 3), generator=gen, dtype=torch.float32, device=dev)).abs() * covered[..., None]
    base = {"mode": "finish", "mesh": "drone", "width": size, "height": size, "covered_share": round(float(covered.float().mean()), 4),
            "calls": calls}
    moved = 60 * n                                   # compulsory bytes of one level

    def median_ms(form, levels, dilate):
        ms = []
        for k in range(warmup + calls):
            ctxs[form].lightmap_finish_device(size, size, img.data_ptr(), pts.data_ptr(), nrm.data_ptr(), out[form].data_ptr(), valid.data_ptr(),
                                              levels=levels, dilate=dilate)
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(ctxs[form].last_kernel_ms())
        return float(np.median(ms))

    # the yardstick: a device-to-device copy that reads 30 n and writes 30 n bytes
    src, dst = torch.empty(30 * n, dtype=torch.uint8, device=dev), torch.empty(30 * n, dtype=torch.uint8, device=dev)
    copy_ms = []
    for k in range(warmup + calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if k >= warmup:
            copy_ms.append(e0.elapsed_time(e1))
    copy = float(np.median(copy_ms))
    rows = [dict(base, query="device-to-device copy of the same byte count", bytes_moved=moved, ms_median=round(copy, 4),
                 gb_per_s=round(moved / copy / 1e6, 1))]
    print(json.dumps(rows[-1]), flush=True)
    del src, dst
    totals = {form: [median_ms(form, k, 0) for k in range(FINISH_LEVELS + 1)] for form in ("direct", "lds")}
    for level in range(FINISH_LEVELS):
        step = 1 << level
        row = dict(base, query=f"lmf_atrous level {level}", step=step, bytes_moved=moved)
        for form in ("direct", "lds"):
            if form == "lds" and step > 8:
                continue
            ms = totals[form][level + 1] - totals[form][level]
            row[f"{form}_ms"] = round(ms, 4)
            row[f"{form}_gb_per_s"] = round(moved / ms / 1e6, 1) if ms > 0 else None
        row["copy_gb_per_s"] = rows[0]["gb_per_s"]
        rows.append(row)
        print(json.dumps(row), flush=True)
    for form in ("direct", "lds"):
        full = median_ms(form, FINISH_LEVELS, FINISH_DILATE)
        rows.append(dict(base, query=f"whole call, every step {form} (step 16: direct)", levels=FINISH_LEVELS, dilate=FINISH_DILATE,
                         ms_median=round(full, 4), lmf_mask_ms=round(totals[form][0], 4),
                         lmf_dilate_ms_per_pass=round((full - totals[form][FINISH_LEVELS]) / FINISH_DILATE, 4)))
        print(json.dumps(rows[-1]), flush=True)
    full = median_ms("default", FINISH_LEVELS, FINISH_DILATE)
    rows.append(dict(base, query="whole call, the library's threshold", levels=FINISH_LEVELS, dilate=FINISH_DILATE, ms_median=round(full, 4)))
    print(json.dumps(rows[-1]), flush=True)
    same = bool(torch.equal(out["direct"].view(torch.int32), out["lds"].view(torch.int32)) and
                torch.equal(out["direct"].view(torch.int32), out["default"].view(torch.int32)))
    rows.append(dict(base, query="direct and LDS forms give the same bits", same=same))
    print(json.dumps(rows[-1]), flush=True)
    for c in ctxs.values():
        c.close()
    if not same:
        raise SystemExit("ray_query_bench: the LDS and the direct form of lmf_atrous differ")
    return rows


def occlusion_rows(ctx, cfg, sc, co, cd, bo, bd, hitpoints, calls, warmup):
    to = (np.array(SHADOW_POINT, np.float32) - hitpoints).astype(np.float32)
    dist = np.sqrt((to.astype(np.float64) ** 2).sum(axis=1))
    ok = dist > 2e-3
    so = np.ascontiguousarray(hitpoints[ok])
    sd = np.ascontiguousarray((to[ok] / dist[ok, None]).astype(np.float32))
    stm = np.ascontiguousarray((dist[ok] - 1e-3).astype(np.float32))
    rows = []
    for set_name, o, d, t_max, tm in (("camera", co, cd, sc.camera.max_trace_dist, None), ("bounce", bo, bd, float("inf"), None),
                                      ("shadow", so, sd, float("inf"), stm)):
        for r in measure_pair(ctx, o, d, t_max, tm, calls, warmup):
            row = dict({"config": cfg, "rays": set_name, "n_rays": len(o), "calls": calls}, **r)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def render_rows(ctx, cfg, sc, co, cd, calls, warmup):
    """mi_shade_rays_device on the pixel-centre rays, then mi_render_rays_device on the same rays as a one-row table, at 1 and 16 spp."""
    from cs397raytracingsp22_amd import dist as pdist
    dev = torch.device("cuda:0")
    cam = sc.camera
    W, H = cam.screen_width, cam.screen_height
    n = len(co)
    assert n == W * H
    t_o, t_d = torch.from_numpy(co).to(dev), torch.from_numpy(cd).to(dev)          # [H*W, 3] row-major = a table [1][H][W][3]
    t_rgb = torch.empty((n, 3), dtype=torch.float32, device=dev)
    t_compact = torch.empty((pdist.tiles_padded(W, H, 1) * pdist.TILE_PIXELS, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def timed(call):
        ms = []
        for k in range(warmup + calls):
            call()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(ctx.last_kernel_ms())
        return ms

    rows = []

    def report(query, aa, ms, extra):
        med = float(np.median(ms))
        row = dict({"config": cfg, "mode": "render", "query": query, "n_rays": n, "aa_sample_count": aa, "path_depth": cam.path_depth,
                    "calls": calls, "kernel_ms_median": round(med, 4), "kernel_ms_min": round(float(np.min(ms)), 4),
                    "kernel_ms_max": round(float(np.max(ms)), 4), "msamples_per_s_kernel": round(n * aa / med / 1e3, 1)}, **extra)
        rows.append(row)
        print(json.dumps(row), flush=True)

    cam.aa_sample_count = 1
    ms = timed(lambda: ctx.shade_rays_device(cam, n, t_o.data_ptr(), t_d.data_ptr(), t_rgb.data_ptr(), seed=1, first_key=0))
    report("shade_rays", 1, ms, {"mean_radiance": round(float(t_rgb.mean().item()), 6)})
    for aa in (1, 16):
        cam.aa_sample_count = aa
        ms = timed(lambda: ctx.render_rays_device(cam, t_o.data_ptr(), t_d.data_ptr(), 1, t_compact.data_ptr(), seed=1))
        report("render_rays", aa, ms, {"mean_radiance_compact": round(float(t_compact.mean().item()), 6),
                                       "segments": ctx.last_pipeline_counts()["segments"]})
    return rows


def volume_rows(ctx, grids, point_counts, calls, warmup):
    """--mode volume (the module's docstring)"""
    from cs397raytracingsp22_amd import probe_volume_sample
    dev = torch.device("cuda:0")
    size = 4096
    sc = scenes.config4(size, size, 1, 10)
    drone = sc.objects[-1]
    mesh = drone.mesh
    t_mesh = [torch.from_numpy(np.array(a)).to(dev) for a in (mesh.positions, mesh.normals, mesh.texcoords, mesh.indices.view(np.int32))]
    pts = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
    ctx.lightmap_texels_device(t_mesh[0].data_ptr(), t_mesh[1].data_ptr(), t_mesh[2].data_ptr(), t_mesh[3].data_ptr(), mesh.n_vertices,
                               mesh.n_triangles, size, size, pts.data_ptr(), nrm.data_ptr(), None, rows=1, jitter=False, seed=1,
                               offset=float(np.float32(1e-3)), transform=drone.transform)
    torch.cuda.synchronize()
    covered = (nrm != 0).any(dim=-1).reshape(-1)
    all_p, all_n = pts.reshape(-1, 3)[covered], nrm.reshape(-1, 3)[covered]                  # raster order
    del pts, nrm
    lo = (all_p.min(dim=0).values - 0.05).cpu().numpy().astype(np.float32)
    hi = (all_p.max(dim=0).values + 0.05).cpu().numpy().astype(np.float32)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    rows = []
    for n_points in point_counts:
        reps = (n_points + len(all_p) - 1) // len(all_p)
        coh_p, coh_n = all_p.repeat(reps, 1)[:n_points].contiguous(), all_n.repeat(reps, 1)[:n_points].contiguous()
        perm = torch.randperm(n_points, generator=gen, device=dev)
        sets = {"coherent": (coh_p, coh_n), "incoherent": (coh_p[perm].contiguous(), coh_n[perm].contiguous())}
        out_E = torch.empty((n_points, 3), dtype=torch.float32, device=dev)
        out_w = torch.empty(n_points, dtype=torch.float32, device=dev)
        moved = 40 * n_points
        src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_ms = []
        for k in range(warmup + calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                copy_ms.append(e0.elapsed_time(e1))
        copy = float(np.median(copy_ms))
        del src, dst
        for g in grids:
            n_probes = g ** 3
            sh_host = np.random.default_rng(g).normal(0.0, 1.0, (n_probes, 9, 3)).astype(np.float32)
            sh_host[:, 0, :] += 3.0
            valid_host = (np.arange(n_probes) % 5 != 0).astype(np.uint8)
            sh, valid = torch.from_numpy(sh_host).to(dev), torch.from_numpy(valid_host).to(dev)

            def timed(p, nn, n):
                ms = []
                for k in range(warmup + calls):
                    ctx.probe_volume_sample_device(lo, hi, (g, g, g), sh.data_ptr(), n, p.data_ptr(), nn.data_ptr(), out_E.data_ptr(),
                                                   d_weight=out_w.data_ptr(), d_valid=valid.data_ptr(), flags=abi.MI_PV_NORMAL_WEIGHT)
                    torch.cuda.synchronize()
                    if k >= warmup:
                        ms.append(ctx.last_kernel_ms())
                return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))

            prep = timed(coh_p, coh_n, 1)
            for name, (p, nn) in sets.items():
                med, mn, mx = timed(p, nn, n_points)
                k = min(4096, n_points)
                want_E, want_w = probe_volume_sample(lo, hi, (g, g, g), sh_host, p[:k].cpu().numpy(), nn[:k].cpu().numpy(), valid_host,
                                                     abi.MI_PV_NORMAL_WEIGHT)
                got_E, got_w = out_E[:k].cpu().numpy(), out_w[:k].cpu().numpy()
                differ = int(((got_E.view(np.uint32) != want_E.view(np.uint32)).any(axis=-1) | (got_w.view(np.uint32) != want_w.view(np.uint32))).sum())
                row = {"mode": "volume", "grid": g, "record_bytes": 112 * n_probes, "n_points": n_points, "points": name, "calls": calls,
                       "kernel_ms_median": round(med, 4), "kernel_ms_min": round(mn, 4), "kernel_ms_max": round(mx, 4),
                       "pv_prepare_ms_median": round(prep[0], 4), "mpoints_per_s": round(n_points / med / 1e3, 1),
                       "gb_per_s_on_40_bytes": round(moved / med / 1e6, 1), "copy_ms_median": round(copy, 4),
                       "copy_gb_per_s": round(moved / copy / 1e6, 1), "checked_points": k, "differ_from_helper": differ}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return rows


def variance_rows(ctx, sizes, calls, warmup):
    """--mode variance (the module's docstring)"""
    from cs397raytracingsp22_amd import dist as pdist
    dev = torch.device("cuda:0")
    offset = float(np.float32(1e-3))
    rows = []

    def atlas(size, aa):
        sc = scenes.config4(size, size, aa, 10)
        drone = sc.objects[-1]
        mesh = drone.mesh
        t_mesh = [torch.from_numpy(np.array(a)).to(dev) for a in (mesh.positions, mesh.normals, mesh.texcoords, mesh.indices.view(np.int32))]
        pts = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        nrm = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        ctx.lightmap_texels_device(t_mesh[0].data_ptr(), t_mesh[1].data_ptr(), t_mesh[2].data_ptr(), t_mesh[3].data_ptr(), mesh.n_vertices,
                                   mesh.n_triangles, size, size, pts.data_ptr(), nrm.data_ptr(), None, rows=1, jitter=False, seed=1,
                                   offset=offset, transform=drone.transform)
        torch.cuda.synchronize()
        return sc, pts, nrm

    def stats(ms):
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}

    # 1. the moments
    size = 1024
    sc, pts, nrm = atlas(size, BAKE_AA)
    cam = sc.camera
    ctx.upload(sc.flatten())
    slots = pdist.tiles_padded(size, size, 1) * pdist.TILE_PIXELS
    c_plain = torch.empty((slots, 3), dtype=torch.float32, device=dev)
    c_mom = torch.empty((slots, 3), dtype=torch.float32, device=dev)
    c_m2 = torch.empty((slots, 3), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ms = {"plain": [], "moments": []}
    reduce_ms = {"plain": [], "moments": []}
    m2_ms = []
    for k in range(warmup + calls):
        ctx.render_points_moments_device(cam, pts.data_ptr(), nrm.data_ptr(), 1, c_m2.data_ptr(), c_mom.data_ptr(), seed=1)
        torch.cuda.synchronize()
        if k >= warmup:
            ms["moments"].append(ctx.last_kernel_ms())
            reduce_ms["moments"].append(ctx.last_pipeline_ms()["wf_reduce_ms"])
            m2_ms.append(ctx.last_reduce_m2_ms())
        ctx.render_points_device(cam, pts.data_ptr(), nrm.data_ptr(), 1, c_plain.data_ptr(), seed=1)
        torch.cuda.synchronize()
        if k >= warmup:
            ms["plain"].append(ctx.last_kernel_ms())
            reduce_ms["plain"].append(ctx.last_pipeline_ms()["wf_reduce_ms"])
    same = bool(torch.equal(c_plain.view(torch.int32), c_mom.view(torch.int32)))
    base = {"mode": "variance", "mesh": "drone", "width": size, "height": size, "aa_sample_count": BAKE_AA, "path_depth": cam.path_depth,
            "covered_share": round(float((nrm != 0).any(dim=-1).float().mean()), 4), "calls": calls}
    rows.append(dict(base, query="mi_render_points_device", **stats(ms["plain"]), wf_reduce_ms_median=round(float(np.median(reduce_ms["plain"])), 4)))
    rows.append(dict(base, query="mi_render_points_moments_device", **stats(ms["moments"]),
                     wf_reduce_ms_median=round(float(np.median(reduce_ms["moments"])), 4), wf_reduce_m2_ms_median=round(float(np.median(m2_ms)), 4),
                     wf_reduce_m2_ms_min=round(float(np.min(m2_ms)), 4), wf_reduce_m2_ms_max=round(float(np.max(m2_ms)), 4),
                     mean_of_squares=round(float(c_m2.mean().item()), 6)))
    rows.append(dict(base, query="ratio moments / plain", ms_median=round(float(np.median(ms["moments"])) / float(np.median(ms["plain"])), 4),
                     wf_reduce_m2_over_wf_reduce=round(float(np.median(m2_ms)) / float(np.median(reduce_ms["moments"])), 3),
                     compact_images_bit_identical=same))
    for row in rows[-3:]:
        print(json.dumps(row), flush=True)
    if not same:
        raise SystemExit("ray_query_bench: the moments call's image differs from mi_render_points_device's")
    del c_plain, c_mom, c_m2, pts, nrm

    # 2. the finish
    for size in sizes:
        _, pts, nrm = atlas(size, 1)
        covered = (nrm != 0).any(dim=-1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        img = (1.0 + 0.5 * torch.randn((size, size, 3), generator=gen, dtype=torch.float32, device=dev)).abs() * covered[..., None]
        sd = 0.3 * img * (0.5 + torch.rand((size, size, 3), generator=gen, dtype=torch.float32, device=dev))
        m2 = img * img + sd * sd * ((BAKE_AA - 1) / BAKE_AA)
        out = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        var = torch.empty((size, size), dtype=torch.float32, device=dev)
        valid = torch.empty((size, size), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = {"fixed": [], "variance": []}
        for k in range(warmup + calls):
            ctx.lightmap_finish_device(size, size, img.data_ptr(), pts.data_ptr(), nrm.data_ptr(), out.data_ptr(), valid.data_ptr(),
                                       levels=FINISH_LEVELS, sigma_color=8.0, dilate=FINISH_DILATE)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["fixed"].append(ctx.last_kernel_ms())
            ctx.lightmap_finish_var_device(size, size, img.data_ptr(), m2.data_ptr(), BAKE_AA, pts.data_ptr(), nrm.data_ptr(), out.data_ptr(),
                                           var.data_ptr(), valid.data_ptr(), levels=FINISH_LEVELS, sigma_color=8.0, color_floor=1e-6,
                                           dilate=FINISH_DILATE)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["variance"].append(ctx.last_kernel_ms())
        base = {"mode": "variance", "mesh": "drone", "width": size, "height": size, "levels": FINISH_LEVELS, "dilate": FINISH_DILATE,
                "covered_share": round(float(covered.float().mean()), 4), "calls": calls}
        rows.append(dict(base, query="mi_lightmap_finish_device", **stats(ms["fixed"])))
        rows.append(dict(base, query="mi_lightmap_finish_var_device", **stats(ms["variance"]),
                         mean_variance=float(var.mean().item())))
        rows.append(dict(base, query="ratio variance-guided / fixed",
                         ms_median=round(float(np.median(ms["variance"])) / float(np.median(ms["fixed"])), 4)))
        for row in rows[-3:]:
            print(json.dumps(row), flush=True)
        del pts, nrm, img, sd, m2, out, var, valid
    return rows


def adaptive_rows(ctx, size, bakes, first=16, per_round=16, rounds=2):
    """--mode adaptive (the module's docstring)"""
    from dataclasses import replace
    from cs397raytracingsp22_amd import Lambertian, Scene, StaticMesh, cgmath, lightmap_select, objload
    dev = torch.device("cuda:0")
    offset = float(np.float32(1e-3))
    rows = []
    drone_scene = scenes.config4(size, size, first, 10)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import gzip
    with gzip.open(os.path.join(root, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
        cube = objload.load_obj_text(fh.read())[0]
    xf = cgmath.mul(cgmath.from_translation((0.2, 1.6, -0.3)), cgmath.from_angle_y(25.0), cgmath.from_scale(0.8))
    box = StaticMesh(cube, Lambertian(albedo=(0.7, 0.7, 0.7)), [None] * 5, xf)
    box_scene = Scene(replace(drone_scene.camera, path_depth=6), scenes.cornell_walls() + [box])
    for name, sc, mesh in (("cube-in-box", box_scene, box), ("drone", drone_scene, drone_scene.objects[-1])):
        cam = replace(sc.camera, screen_width=size, screen_height=size, aa_sample_count=first)
        ctx.upload(sc.flatten())
        # the targets: the median of the first round's error over its luminance, so that round 1 takes about half of the lit texels
        m2_0, f32_0, _, _, _, _ = ctx.bake_lightmap_moments(cam, mesh, offset=offset, seed=1, want_u8=False)
        _, normals, _ = ctx.lightmap_texels(mesh, size, size, rows=1, offset=offset, want_triangle=False)
        covered = (normals[0] != 0).any(axis=-1)
        counts_0 = np.full((size, size), first, np.uint32)
        _, _, err = lightmap_select(f32_0, m2_0, counts_0, normals[0], 0.0, 0.0)
        lum = np.abs(f32_0).sum(axis=-1)
        lit = covered & (lum > 0) & (err > 0)
        trel = float(np.float32(np.median(err[lit] / lum[lit])))
        total_b = first + rounds * per_round
        ref = ctx.bake_lightmap_moments(replace(cam, aa_sample_count=16 * total_b), mesh, offset=offset, seed=977, want_u8=False)[1]

        def error(img):            # mean absolute error per channel, and the mean of the texel's error over its luminance (+ 1e-3)
            d = np.abs(img.astype(np.float64) - ref)
            return {"mean_abs_error": round(float(d[covered].mean()), 6),
                    "mean_rel_error": round(float((d.sum(axis=-1) / (np.abs(ref).sum(axis=-1) + 1e-3))[covered].mean()), 6)}

        ms, st = [], None
        for k in range(bakes + 1):
            counts, _, f32_a, _, _, _, st = ctx.bake_lightmap_adaptive(cam, mesh, first, per_round, rounds, trel, 0.0, offset=offset, seed=1,
                                                                       want_u8=False)
            if k:
                ms.append(st.total_ms)
        total_a = max(first, int(round(st.samples / (size * size))))
        base = {"mode": "adaptive", "mesh": name, "width": size, "height": size, "first_samples": first, "round_samples": per_round,
                "max_rounds": rounds, "target_rel": round(trel, 5), "covered_share": round(float(covered.mean()), 4), "bakes": bakes}
        rows.append(dict(base, query="mi_bake_lightmap_adaptive", ms_median=round(float(np.median(ms)), 3), ms_min=round(float(np.min(ms)), 3),
                         ms_max=round(float(np.max(ms)), 3), slots=int(st.samples), slots_per_texel=round(st.samples / (size * size), 3),
                         mean_count_covered=round(float(counts[covered].mean()), 3), refined_share=round(float((counts[covered] > first).mean()), 4),
                         **error(f32_a)))
        print(json.dumps(rows[-1]), flush=True)
        for what, spp in (("the adaptive run's slots per texel", total_a), ("first + max_rounds * round_samples", total_b)):
            ms_u, f32_u = [], None
            for k in range(bakes + 1):
                _, f32_u, _, _, _, st_u = ctx.bake_lightmap_moments(replace(cam, aa_sample_count=spp), mesh, offset=offset, seed=1, want_u8=False)
                if k:
                    ms_u.append(st_u.total_ms)
            rows.append(dict(base, query=f"mi_bake_lightmap_moments at {spp} samples ({what})", ms_median=round(float(np.median(ms_u)), 3),
                             ms_min=round(float(np.min(ms_u)), 3), ms_max=round(float(np.max(ms_u)), 3), **error(f32_u)))
            print(json.dumps(rows[-1]), flush=True)
        # the bookkeeping of round 1 beside its render: device forms on resident tables, HIP events
        index, count, _ = ctx.lightmap_select(f32_0, m2_0, counts_0, normals[0], trel, 0.0, want_error=False)
        jp, jn, _ = ctx.lightmap_texels(mesh, size, size, rows=per_round, jitter=True, seed=2, offset=offset, want_triangle=False)
        t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (f32_0, m2_0, counts_0.view(np.int32), normals[0], jp, jn)]
        n, cw = int(index.size), 1024
        ch = (n + cw - 1) // cw
        d_index = torch.empty((size * size,), dtype=torch.int32, device=dev)
        d_count = torch.zeros((1,), dtype=torch.int32, device=dev)
        tp = torch.empty((per_round, ch, cw, 3), dtype=torch.float32, device=dev)
        tn = torch.empty((per_round, ch, cw, 3), dtype=torch.float32, device=dev)
        camr = replace(cam, screen_width=cw, screen_height=ch, aa_sample_count=per_round)
        part = {"select": [], "gather": [], "merge": [], "render": []}
        for k in range(bakes + 1):
            torch.cuda.synchronize()
            ctx.lightmap_select_device(size, size, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), trel, 0.0, size * size,
                                       d_index.data_ptr(), d_count.data_ptr())
            torch.cuda.synchronize()
            sel = ctx.last_kernel_ms()
            ctx.lightmap_gather_device(size, size, per_round, n, d_index.data_ptr(), t[4].data_ptr(), t[5].data_ptr(), cw, tp.data_ptr(), tn.data_ptr())
            torch.cuda.synchronize()
            gat = ctx.last_kernel_ms()
            rm2, rmean, _, _, rst = ctx.render_points_moments(camr, tp.cpu().numpy(), tn.cpu().numpy(), seed=2, want_u8=False)
            t_mean, t_rm2 = torch.from_numpy(rmean).to(dev), torch.from_numpy(rm2).to(dev)
            img, m2c, cnt = t[0].clone(), t[1].clone(), t[2].clone()
            torch.cuda.synchronize()
            ctx.lightmap_merge_device(size, size, n, d_index.data_ptr(), t_mean.data_ptr(), t_rm2.data_ptr(), per_round, img.data_ptr(),
                                      m2c.data_ptr(), cnt.data_ptr())
            torch.cuda.synchronize()
            if k:
                for key, v in (("select", sel), ("gather", gat), ("merge", ctx.last_kernel_ms()), ("render", rst.kernel_ms)):
                    part[key].append(v)
        med = {k: float(np.median(v)) for k, v in part.items()}
        book = med["select"] + med["gather"] + med["merge"]
        assert int(d_count.item()) == count == n
        rows.append(dict(base, query="round 1: select + gather + merge beside the render", selected=n,
                         **{f"{k}_ms_median": round(v, 4) for k, v in med.items()}, bookkeeping_share_of_round=round(book / (book + med["render"]), 4)))
        print(json.dumps(rows[-1]), flush=True)
        del t, tp, tn, d_index
    return rows


def directional_rows(ctx, sizes, point_counts, calls, warmup):
    """--mode directional: the three measurements of the directional lightmap calls on device-resident tables, HIP events, `warmup`
    warm-up and `calls` timed calls, medians (min - max beside them).
    Bake: the drone's atlas at 1024 x 1024 (mi_lightmap_texels_device's centre table), path_depth 10, aa_sample_count 16 and 64:
    mi_render_points_sh_device alternates call by call with mi_render_points_device; the rows give mi_last_kernel_ms of each, wf_reduce_psh
    (entry 7 of mi_last_pipeline_ms) and its share of the call, and beside it wf_reduce_sh's time and share in a mi_render_probes_device
    render of the same points and sample count (equal slot count).  The tool checks that the two compact images agree bit for bit.
    Finish: at --finish-sizes, levels = 5 and dilate = 8, mi_lightmap_finish_sh_device on seeded records against NINE
    mi_lightmap_finish_device calls on the nine planes, both with sigma_color = +inf, and checks that they give the same bits.
    Evaluation: mi_lightmap_sh_eval_device at --volume-points points (132 B per point: 108 + 12 in, 12 out) against a device-to-device
    copy of the same byte count timed in the same run.
    Measured on one MI355X (DESIGN.md "Directional lightmaps" has the table and the reading):
      wf_reduce_psh: 0.153 ms of a 13.74 ms bake at 16 samples (1.1 %), 0.574 ms of 45.72 ms at 64 (1.3 %); the plain bakes take 13.59
        and 45.17 ms, so the SH bake costs 1.011 x and 1.012 x.  wf_reduce_sh in a probes render of the same slots: 0.134 ms of 26.4 ms
        and 0.495 ms of 96.9 ms (0.5 %): wf_reduce_psh takes 1.14 x and 1.16 x wf_reduce_sh's time.
      finish, levels 5 and dilate 8: 1024^2 2.03 ms against 5.23 ms for the nine calls (0.39 x); 2048^2 6.80 ms against 12.40 ms (0.55 x)
      eval: 2^20 points 0.024 ms = 5.7 TB/s (the copy of the same 138 MB: 5.2 TB/s; both from the Infinity Cache);
        2^22 points 0.115 ms = 4.8 TB/s (the copy of the same 554 MB: 5.7 TB/s), 0.60 of the 8 TB/s roof bench.py accounts against"""
    from cs397raytracingsp22_amd import dist as pdist
    dev = torch.device("cuda:0")
    offset = float(np.float32(1e-3))
    rows = []

    def atlas(size, aa):
        sc = scenes.config4(size, size, aa, 10)
        drone = sc.objects[-1]
        mesh = drone.mesh
        t_mesh = [torch.from_numpy(np.array(a)).to(dev) for a in (mesh.positions, mesh.normals, mesh.texcoords, mesh.indices.view(np.int32))]
        pts = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        nrm = torch.empty((size, size, 3), dtype=torch.float32, device=dev)
        ctx.lightmap_texels_device(t_mesh[0].data_ptr(), t_mesh[1].data_ptr(), t_mesh[2].data_ptr(), t_mesh[3].data_ptr(), mesh.n_vertices,
                                   mesh.n_triangles, size, size, pts.data_ptr(), nrm.data_ptr(), None, rows=1, jitter=False, seed=1,
                                   offset=offset, transform=drone.transform)
        torch.cuda.synchronize()
        return sc, pts, nrm

    def stats(ms, key="ms"):
        return {f"{key}_median": round(float(np.median(ms)), 4), f"{key}_min": round(float(np.min(ms)), 4), f"{key}_max": round(float(np.max(ms)), 4)}

    # 1. wf_reduce_psh
    size = 1024
    slots = pdist.tiles_padded(size, size, 1) * pdist.TILE_PIXELS
    for aa in (16, 64):
        sc, pts, nrm = atlas(size, aa)
        cam = sc.camera
        ctx.upload(sc.flatten())
        c_plain = torch.empty((slots, 3), dtype=torch.float32, device=dev)
        c_sh3 = torch.empty((slots, 3), dtype=torch.float32, device=dev)
        c_sh = torch.empty((slots, 27), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ms = {"plain": [], "sh": [], "probes": []}
        red = {"psh": [], "probes_sh": [], "wf_reduce": []}
        for k in range(warmup + calls):
            ctx.render_points_sh_device(cam, pts.data_ptr(), nrm.data_ptr(), 1, c_sh.data_ptr(), c_sh3.data_ptr(), seed=1)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["sh"].append(ctx.last_kernel_ms())
                red["psh"].append(ctx.last_reduce_psh_ms())
                red["wf_reduce"].append(ctx.last_pipeline_ms()["wf_reduce_ms"])
            ctx.render_points_device(cam, pts.data_ptr(), nrm.data_ptr(), 1, c_plain.data_ptr(), seed=1)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["plain"].append(ctx.last_kernel_ms())
        same = bool(torch.equal(c_plain.view(torch.int32), c_sh3.view(torch.int32)))
        for k in range(warmup + calls):                      # the kernel it is modelled on: the same points as probes, equal slot count
            ctx.render_probes_device(cam, pts.data_ptr(), 1, c_sh.data_ptr(), c_sh3.data_ptr(), seed=1)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["probes"].append(ctx.last_kernel_ms())
                red["probes_sh"].append(ctx.last_reduce_sh_ms())
        base = {"mode": "directional", "mesh": "drone", "width": size, "height": size, "aa_sample_count": aa, "path_depth": cam.path_depth,
                "covered_share": round(float((nrm != 0).any(dim=-1).float().mean()), 4), "calls": calls}
        psh, plain, sh_ms = float(np.median(red["psh"])), float(np.median(ms["plain"])), float(np.median(ms["sh"]))
        prb, prb_sh = float(np.median(ms["probes"])), float(np.median(red["probes_sh"]))
        rows.append(dict(base, query="mi_render_points_device", **stats(ms["plain"])))
        rows.append(dict(base, query="mi_render_points_sh_device", **stats(ms["sh"]), **stats(red["psh"], "wf_reduce_psh_ms"),
                         wf_reduce_ms_median=round(float(np.median(red["wf_reduce"])), 4), wf_reduce_psh_share=round(psh / sh_ms, 5),
                         sh_over_plain=round(sh_ms / plain, 4), compact_images_bit_identical=same))
        rows.append(dict(base, query="mi_render_probes_device, the same points", **stats(ms["probes"]), **stats(red["probes_sh"], "wf_reduce_sh_ms"),
                         wf_reduce_sh_share=round(prb_sh / prb, 5), wf_reduce_psh_over_wf_reduce_sh=round(psh / prb_sh, 3)))
        for row in rows[-3:]:
            print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("ray_query_bench: the SH call's image differs from mi_render_points_device's")
        del c_plain, c_sh3, c_sh, pts, nrm

    # 2. the finish: one call on 27 channels against nine calls on three
    for size in sizes:
        _, pts, nrm = atlas(size, 1)
        covered = (nrm != 0).any(dim=-1)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        rec = torch.randn((size, size, 9, 3), generator=gen, dtype=torch.float32, device=dev) * covered[..., None, None]
        planes = [rec[:, :, k, :].contiguous() for k in range(9)]
        out = torch.empty((size, size, 9, 3), dtype=torch.float32, device=dev)
        out3 = [torch.empty((size, size, 3), dtype=torch.float32, device=dev) for _ in range(9)]
        valid = torch.empty((size, size), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms = {"one": [], "nine": []}
        for k in range(warmup + calls):
            ctx.lightmap_finish_sh_device(size, size, rec.data_ptr(), pts.data_ptr(), nrm.data_ptr(), out.data_ptr(), valid.data_ptr(),
                                          levels=FINISH_LEVELS, dilate=FINISH_DILATE)
            torch.cuda.synchronize()
            if k >= warmup:
                ms["one"].append(ctx.last_kernel_ms())
            total = 0.0
            for j in range(9):
                ctx.lightmap_finish_device(size, size, planes[j].data_ptr(), pts.data_ptr(), nrm.data_ptr(), out3[j].data_ptr(), valid.data_ptr(),
                                           levels=FINISH_LEVELS, dilate=FINISH_DILATE)
                torch.cuda.synchronize()
                total += ctx.last_kernel_ms()
            if k >= warmup:
                ms["nine"].append(total)
        same = all(bool(torch.equal(out[:, :, j, :].contiguous().view(torch.int32), out3[j].view(torch.int32))) for j in range(9))
        base = {"mode": "directional", "mesh": "drone", "width": size, "height": size, "levels": FINISH_LEVELS, "dilate": FINISH_DILATE,
                "covered_share": round(float(covered.float().mean()), 4), "calls": calls}
        rows.append(dict(base, query="mi_lightmap_finish_sh_device", **stats(ms["one"])))
        rows.append(dict(base, query="nine mi_lightmap_finish_device calls", **stats(ms["nine"])))
        rows.append(dict(base, query="ratio one call / nine calls", ms_median=round(float(np.median(ms["one"])) / float(np.median(ms["nine"])), 4),
                         same_bits=same))
        for row in rows[-3:]:
            print(json.dumps(row), flush=True)
        if not same:
            raise SystemExit("ray_query_bench: mi_lightmap_finish_sh_device differs from mi_lightmap_finish_device plane by plane")
        del pts, nrm, rec, planes, out, out3, valid

    # 3. the evaluation
    for n in point_counts:
        gen = torch.Generator(device=dev)
        gen.manual_seed(2)
        rec = torch.randn((n, 9, 3), generator=gen, dtype=torch.float32, device=dev)
        nrm = torch.randn((n, 3), generator=gen, dtype=torch.float32, device=dev)
        E = torch.empty((n, 3), dtype=torch.float32, device=dev)
        src, dst = torch.empty(66 * n, dtype=torch.uint8, device=dev), torch.empty(66 * n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ms, copy_ms = [], []
        for k in range(warmup + calls):
            ctx.lightmap_sh_eval_device(n, rec.data_ptr(), nrm.data_ptr(), E.data_ptr())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            if k >= warmup:
                ms.append(ctx.last_kernel_ms())
                copy_ms.append(e0.elapsed_time(e1))
        moved = 132 * n
        rows.append(dict(mode="directional", query="mi_lightmap_sh_eval_device", n_points=n, bytes_moved=moved, calls=calls, **stats(ms),
                         gb_per_s=round(moved / float(np.median(ms)) / 1e6, 1), copy_ms_median=round(float(np.median(copy_ms)), 4),
                         copy_gb_per_s=round(moved / float(np.median(copy_ms)) / 1e6, 1)))
        print(json.dumps(rows[-1]), flush=True)
        del rec, nrm, E, src, dst
    return rows


def lookup_rows(ctx, sizes, point_counts, calls, warmup):
    """--mode lookup: the lightmap lookup kernels on resident tables, HIP events inside the library (mi_last_kernel_ms), `warmup` calls
    then `calls` timed ones, medians with min - max.  Inputs: a seeded random SH lightmap [size, size, 9, 3] (all texels valid) and a
    3-channel image of the same size, for size in `sizes`; n points for n in `point_counts`, unit normals.  The uv come in two orders:
    "coherent" — the first n points, row-major, of the atlas's own grid at twice its resolution (neighbouring lanes share their taps;
    the points span n / 4 texels, 113 MB of records at 2^22) — and "shuffled", n points of that grid drawn at random over the WHOLE
    table (113 MB of records at 1024^2, 453 MB at 2048^2).  Rows per (size, n, order): lml_sample<3>, lml_sample<27>,
    lml_sh_sample (the fused form), the composition lml_sample<27> + lsh_eval (the sum of the two kernels' times), and a device-to-device
    copy of the fused form's nominal byte count (per point 8 + 12 in, four 108-byte taps, 12 + 4 out = 468 bytes, half of it copied:
    read and written).  The results are checked against lightmap_sample / lightmap_sh_sample on a 4096-point subsample, bit for bit.
    The measured figures are in DESIGN.md section 4, "Lightmap lookup"."""
    from cs397raytracingsp22_amd import lightmap_sample, lightmap_sh_sample
    dev = torch.device("cuda:0")
    rows = []

    def stats(ms):
        return {"ms_median": round(float(np.median(ms)), 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4)}

    def bits(t):
        return t.contiguous().view(torch.int32).cpu().numpy()

    for size in sizes:
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        sh = torch.randn((size, size, 9, 3), generator=gen, dtype=torch.float32, device=dev)
        img = torch.randn((size, size, 3), generator=gen, dtype=torch.float32, device=dev)
        sh_host, img_host = sh.cpu().numpy(), img.cpu().numpy()
        for n in point_counts:
            k = torch.arange(n, device=dev, dtype=torch.int64)
            gw = 2 * size
            if n > gw * gw:
                raise SystemExit(f"ray_query_bench: {n} points exceed the {gw} x {gw} grid")
            def centres(k):                  # the uv of the points number k of the gw x gw grid, row-major
                u = ((k % gw).to(torch.float32) + 0.5) / gw
                v = 1.0 - ((k // gw).to(torch.float32) + 0.5) / gw
                return torch.stack([u, v], dim=1).contiguous()

            nrm = torch.randn((n, 3), generator=gen, dtype=torch.float32, device=dev)
            nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
            anywhere = torch.randint(0, gw * gw, (n,), generator=gen, device=dev, dtype=torch.int64)
            out3 = torch.empty((n, 3), dtype=torch.float32, device=dev)
            out27 = torch.empty((n, 27), dtype=torch.float32, device=dev)
            E, E2 = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
            w = torch.empty(n, dtype=torch.float32, device=dev)
            src, dst = torch.empty(234 * n, dtype=torch.uint8, device=dev), torch.empty(234 * n, dtype=torch.uint8, device=dev)
            for order, uv in (("coherent", centres(k)), ("shuffled", centres(anywhere))):
                torch.cuda.synchronize()
                ms = {"lml_sample<3>": [], "lml_sample<27>": [], "lml_sh_sample": [], "lml_sample<27> + lsh_eval": [], "copy": []}
                for it in range(warmup + calls):
                    t = {}
                    ctx.lightmap_sample_device(size, size, 3, img.data_ptr(), n, uv.data_ptr(), out3.data_ptr(), w.data_ptr())
                    torch.cuda.synchronize()
                    t["lml_sample<3>"] = ctx.last_kernel_ms()
                    ctx.lightmap_sample_device(size, size, 27, sh.data_ptr(), n, uv.data_ptr(), out27.data_ptr(), w.data_ptr())
                    torch.cuda.synchronize()
                    t["lml_sample<27>"] = ctx.last_kernel_ms()
                    ctx.lightmap_sh_eval_device(n, out27.data_ptr(), nrm.data_ptr(), E2.data_ptr())
                    torch.cuda.synchronize()
                    t["lml_sample<27> + lsh_eval"] = t["lml_sample<27>"] + ctx.last_kernel_ms()
                    ctx.lightmap_sh_sample_device(size, size, sh.data_ptr(), n, uv.data_ptr(), nrm.data_ptr(), E.data_ptr(), w.data_ptr())
                    torch.cuda.synchronize()
                    t["lml_sh_sample"] = ctx.last_kernel_ms()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    dst.copy_(src)
                    e1.record()
                    torch.cuda.synchronize()
                    t["copy"] = e0.elapsed_time(e1)
                    if it >= warmup:
                        for key, val in t.items():
                            ms[key].append(val)
                # the helpers on a 4096-point subsample
                pick = torch.linspace(0, n - 1, 4096, device=dev).to(torch.int64)
                uv_h, n_h = uv[pick].cpu().numpy(), nrm[pick].cpu().numpy()
                want3, want27 = lightmap_sample(img_host, uv_h)[0], lightmap_sample(sh_host, uv_h)[0]
                wantE, wantw = lightmap_sh_sample(sh_host, uv_h, n_h)
                same = (np.array_equal(bits(out3[pick]), want3.view(np.int32)) and np.array_equal(bits(out27[pick]), want27.view(np.int32))
                        and np.array_equal(bits(E[pick]), wantE.view(np.int32)) and np.array_equal(bits(w[pick]), wantw.view(np.int32)))
                fused, comp = float(np.median(ms["lml_sh_sample"])), float(np.median(ms["lml_sample<27> + lsh_eval"]))
                moved = 468 * n
                for key in ("lml_sample<3>", "lml_sample<27>", "lml_sh_sample", "lml_sample<27> + lsh_eval", "copy"):
                    row = dict(mode="lookup", size=size, n_points=n, order=order, query=key, calls=calls, **stats(ms[key]))
                    if key == "lml_sh_sample":
                        row.update(fused_over_composition=round(fused / comp, 4), nominal_gb_per_s=round(moved / fused / 1e6, 1),
                                   equals_helpers=same)
                    if key == "copy":
                        row.update(bytes_moved=moved, gb_per_s=round(moved / float(np.median(ms["copy"])) / 1e6, 1))
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                if not same:
                    raise SystemExit("ray_query_bench: the lookup kernels differ from lightmap_sample / lightmap_sh_sample")
            del k, anywhere, nrm, out3, out27, E, E2, w, src, dst
        del sh, img, sh_host, img_host
    return rows


def mips_rows(ctx, sizes, point_counts, calls, warmup):
    """--mode mips: the lightmap mip chain on resident tables, HIP events inside the library (mi_last_kernel_ms: the span of a call's
    launches), `warmup` calls then `calls` timed ones, medians with min - max; `spread` is (max - min) / median of a row, the run-to-run
    spread a difference between two rows has to exceed.  Inputs per size and channel count (3, 27): a seeded random image
    [size, size, C] under a chart-and-gutter mask (60 x 60 charts on a 64-texel pitch: 88 % valid).  Rows:
    "fused" — mi_lightmap_mips_device of the full chain as the library launches it by default (five levels per launch from one
    32 x 32 tile); "unfused" — the same call on a context created with MI_RT_LMM_LEVELS_PER_LAUNCH=1 (one level per launch);
    "copy" — a device-to-device copy of the nominal bytes (level 0 and its mask read once; every level's texels, mask and coverage
    written once; half of it copied: read and written).  Both forms are checked against lightmap_mips, every level, bit for bit.
    Then, per point count, the trilinear lookups at lod uniform in 0 .. 4 (fractional: two levels, eight taps) against the level-0
    lookups on the same points, in lookup_rows' two orders, "coherent" and "shuffled"; checked against lightmap_sample_lod /
    lightmap_sh_sample_lod on a 4096-point subsample, bit for bit.  The measured figures are in DESIGN.md section 4, "Lightmap mips"."""
    from cs397raytracingsp22_amd import lightmap_mip_layout, lightmap_mips, lightmap_sample_lod, lightmap_sh_sample_lod
    dev = torch.device("cuda:0")
    knob = "MI_RT_LMM_LEVELS_PER_LAUNCH"
    before = os.environ.get(knob)
    os.environ[knob] = "1"
    unfused = Context(0)
    if before is None:
        del os.environ[knob]
    else:
        os.environ[knob] = before
    rows = []

    def stats(ms):
        med = float(np.median(ms))
        return {"ms_median": round(med, 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4),
                "spread": round((float(np.max(ms)) - float(np.min(ms))) / med, 4)}

    def bits(t):
        return t.contiguous().view(torch.int32).cpu().numpy()

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for size in sizes:
        layout = lightmap_mip_layout(size, size)
        L, made = len(layout), sum(w * h for w, h, _ in layout[1:])
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
        valid = ((xx % 64 < 60) & (yy % 64 < 60)).to(torch.uint8).contiguous()
        valid_host = valid.cpu().numpy()
        chains = {}
        for ch in (3, 27):
            img = torch.randn((size, size, ch), generator=gen, dtype=torch.float32, device=dev)
            mips = torch.empty((made, ch), dtype=torch.float32, device=dev)
            mv = torch.empty(made, dtype=torch.uint8, device=dev)
            cov = torch.empty(made, dtype=torch.float32, device=dev)
            moved = size * size * (4 * ch + 1) + made * (4 * ch + 1 + 4)
            src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            want = lightmap_mips(img.cpu().numpy(), valid_host)
            ms = {"fused": [], "unfused": [], "copy": []}
            same = True
            for it in range(warmup + calls):
                t = {}
                for name, c in (("fused", ctx), ("unfused", unfused)):
                    if it == 0:
                        mips.fill_(-7.0), mv.fill_(77), cov.fill_(-7.0)
                    c.lightmap_mips_device(size, size, ch, img.data_ptr(), L, mips.data_ptr(), mv.data_ptr(), cov.data_ptr(), valid.data_ptr())
                    torch.cuda.synchronize()
                    t[name] = c.last_kernel_ms()
                    if it == 0:                  # every level of both forms against the helper
                        gm, gv, gc = bits(mips), mv.cpu().numpy(), bits(cov)
                        for l, (w, h, o) in enumerate(layout[1:], 1):
                            same = (same and np.array_equal(gm[o:o + w * h].reshape(h, w, ch), want[0][l].view(np.int32))
                                    and np.array_equal(gv[o:o + w * h].reshape(h, w), want[1][l])
                                    and np.array_equal(gc[o:o + w * h].reshape(h, w), want[2][l].view(np.int32)))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                t["copy"] = e0.elapsed_time(e1)
                if it >= warmup:
                    for key, val in t.items():
                        ms[key].append(val)
            fused, unf = float(np.median(ms["fused"])), float(np.median(ms["unfused"]))
            for key in ("fused", "unfused", "copy"):
                row = dict(mode="mips", size=size, channels=ch, levels=L, query=key, calls=calls, **stats(ms[key]))
                if key == "fused":
                    row.update(launches=-(-(L - 1) // 5), fused_over_unfused=round(fused / unf, 4), nominal_gb_per_s=round(moved / fused / 1e6, 1),
                               equals_helper=bool(same))
                if key == "unfused":
                    row.update(launches=L - 1, nominal_gb_per_s=round(moved / unf / 1e6, 1))
                if key == "copy":
                    row.update(bytes_moved=moved, gb_per_s=round(moved / float(np.median(ms["copy"])) / 1e6, 1))
                emit(row)
            if not same:
                raise SystemExit("ray_query_bench: the pyramid differs from lightmap_mips")
            chains[ch] = (img, mips, mv, want)
            del src, dst, cov
        # the trilinear lookups against the level-0 lookups
        img3, mips3, mv3, want3 = chains[3]
        sh, mips27, mv27, want27 = chains[27]
        for n in point_counts:
            gw = 2 * size
            if n > gw * gw:
                raise SystemExit(f"ray_query_bench: {n} points exceed the {gw} x {gw} grid")

            def centres(k):                  # the uv of the points number k of the gw x gw grid, row-major
                u = ((k % gw).to(torch.float32) + 0.5) / gw
                v = 1.0 - ((k // gw).to(torch.float32) + 0.5) / gw
                return torch.stack([u, v], dim=1).contiguous()

            k = torch.arange(n, device=dev, dtype=torch.int64)
            anywhere = torch.randint(0, gw * gw, (n,), generator=gen, device=dev, dtype=torch.int64)
            nrm = torch.randn((n, 3), generator=gen, dtype=torch.float32, device=dev)
            nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
            lod = (torch.rand(n, generator=gen, dtype=torch.float32, device=dev) * 4.0).contiguous()
            out3, out27 = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 27), dtype=torch.float32, device=dev)
            E, w = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty(n, dtype=torch.float32, device=dev)
            b3, b27, bE = torch.empty_like(out3), torch.empty_like(out27), torch.empty_like(E)
            for order, uv in (("coherent", centres(k)), ("shuffled", centres(anywhere))):
                torch.cuda.synchronize()
                calls_ = {
                    "lml_sample_lod<3>": lambda: ctx.lightmap_sample_lod_device(size, size, 3, img3.data_ptr(), L, mips3.data_ptr(), n, uv.data_ptr(),
                                                                                lod.data_ptr(), out3.data_ptr(), w.data_ptr(), valid.data_ptr(), mv3.data_ptr()),
                    "lml_sample_lod<27>": lambda: ctx.lightmap_sample_lod_device(size, size, 27, sh.data_ptr(), L, mips27.data_ptr(), n, uv.data_ptr(),
                                                                                 lod.data_ptr(), out27.data_ptr(), w.data_ptr(), valid.data_ptr(), mv27.data_ptr()),
                    "lml_sh_sample_lod": lambda: ctx.lightmap_sh_sample_lod_device(size, size, sh.data_ptr(), L, mips27.data_ptr(), n, uv.data_ptr(),
                                                                                   nrm.data_ptr(), lod.data_ptr(), E.data_ptr(), w.data_ptr(), valid.data_ptr(),
                                                                                   mv27.data_ptr()),
                    "lml_sample<3>": lambda: ctx.lightmap_sample_device(size, size, 3, img3.data_ptr(), n, uv.data_ptr(), b3.data_ptr(), None, valid.data_ptr()),
                    "lml_sample<27>": lambda: ctx.lightmap_sample_device(size, size, 27, sh.data_ptr(), n, uv.data_ptr(), b27.data_ptr(), None, valid.data_ptr()),
                    "lml_sh_sample": lambda: ctx.lightmap_sh_sample_device(size, size, sh.data_ptr(), n, uv.data_ptr(), nrm.data_ptr(), bE.data_ptr(), None,
                                                                           valid.data_ptr()),
                }
                ms = {key: [] for key in calls_}
                for it in range(warmup + calls):
                    for key, call in calls_.items():
                        call()
                        torch.cuda.synchronize()
                        if it >= warmup:
                            ms[key].append(ctx.last_kernel_ms())
                pick = torch.linspace(0, n - 1, 4096, device=dev).to(torch.int64)
                uv_h, n_h, lod_h = uv[pick].cpu().numpy(), nrm[pick].cpu().numpy(), lod[pick].cpu().numpy()
                g3, g27 = lightmap_sample_lod(want3[0], uv_h, lod_h, want3[1])[0], lightmap_sample_lod(want27[0], uv_h, lod_h, want27[1])[0]
                gE, gw_ = lightmap_sh_sample_lod(want27[0], uv_h, n_h, lod_h, want27[1])
                same = (np.array_equal(bits(out3[pick]), g3.view(np.int32)) and np.array_equal(bits(out27[pick]), g27.view(np.int32))
                        and np.array_equal(bits(E[pick]), gE.view(np.int32)) and np.array_equal(bits(w[pick]), gw_.view(np.int32)))
                for key, base in (("lml_sample_lod<3>", "lml_sample<3>"), ("lml_sample_lod<27>", "lml_sample<27>"), ("lml_sh_sample_lod", "lml_sh_sample")):
                    emit(dict(mode="mips", size=size, n_points=n, order=order, query=base, calls=calls, **stats(ms[base])))
                    emit(dict(mode="mips", size=size, n_points=n, order=order, query=key, calls=calls, **stats(ms[key]),
                              lod_over_level0=round(float(np.median(ms[key])) / float(np.median(ms[base])), 4), equals_helpers=bool(same)))
                if not same:
                    raise SystemExit("ray_query_bench: the trilinear lookups differ from lightmap_sample_lod / lightmap_sh_sample_lod")
            del k, anywhere, nrm, lod, out3, out27, E, w, b3, b27, bE
        del chains
    unfused.close()
    return rows


def packed_rows(ctx, sizes, point_counts, calls, warmup):
    """--mode packed: packed lightmaps on resident tables, HIP events inside the library (mi_last_kernel_ms), `warmup` calls then `calls`
    timed ones, medians with min - max; `spread` is (max - min) / median of a row.  Inputs per size: a seeded random image [size, size, 3]
    in 0 .. 4 and records [size, size, 27] (normal deviates) under mips_rows' chart-and-gutter mask, and their full mip chains
    (mi_lightmap_mips_device).  Rows:
    "lmp_pack" / "lmp_unpack" of level 0 per format and channel count — MI_LP_F16 at 3 and 27, MI_LP_RGB9E5 at 3 — against "copy", a
    device-to-device copy of the same bytes (the f32 texels and the packed ones, half of the sum copied: read and written);
    `over_copy` is the ratio of the medians.  The packed words of the first 65536 texels are checked against lightmap_pack, the
    unpacked ones against lightmap_unpack, bit for bit.
    Then, per point count and in lookup_rows' two orders, "coherent" and "shuffled", every packed lookup against its f32 twin — the f32
    kernel on the texels mi_lightmap_unpack_device made of the same packed bytes, so both sides compute the same values — with lod
    (uniform in 0 .. 4) and without (level 0 alone); `packed_over_f32` is the ratio of the medians, and the two outputs are compared on
    the device, every point, bit for bit.  The measured figures are in DESIGN.md section 4, "Packed lightmaps"."""
    from cs397raytracingsp22_amd import abi, lightmap_mip_layout, lightmap_pack, lightmap_unpack
    dev = torch.device("cuda:0")
    F16, RGB = abi.MI_LP_F16, abi.MI_LP_RGB9E5
    rows = []

    def stats(ms):
        med = float(np.median(ms))
        return {"ms_median": round(med, 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4),
                "spread": round((float(np.max(ms)) - float(np.min(ms))) / med, 4)}

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    def same_bits(a, b):
        return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))

    for size in sizes:
        layout = lightmap_mip_layout(size, size)
        L, made, texels = len(layout), sum(w * h for w, h, _ in layout[1:]), size * size
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
        valid = ((xx % 64 < 60) & (yy % 64 < 60)).to(torch.uint8).contiguous()
        del yy, xx
        stored = {}                                                # (format, channels) -> (packed level 0, packed mips, f32 level 0, f32 mips, mip masks)
        for fmt, ch, name in ((F16, 3, "f16 x 3"), (RGB, 3, "rgb9e5 x 3"), (F16, 27, "f16 x 27")):
            if ch == 3:
                img = (torch.rand((size, size, 3), generator=gen, dtype=torch.float32, device=dev) * 4.0).contiguous()
            else:
                img = torch.randn((size, size, 27), generator=gen, dtype=torch.float32, device=dev)
            mips = torch.empty((made, ch), dtype=torch.float32, device=dev)
            mv = torch.empty(made, dtype=torch.uint8, device=dev)
            ctx.lightmap_mips_device(size, size, ch, img.data_ptr(), L, mips.data_ptr(), mv.data_ptr(), None, valid.data_ptr())
            words = (lambda count: torch.empty(count * ch, dtype=torch.int16, device=dev)) if fmt == F16 else (lambda count: torch.empty(count, dtype=torch.int32, device=dev))
            p0, pm = words(texels), words(made)
            u0, um = torch.empty_like(img), torch.empty_like(mips)
            moved = texels * 4 * ch + p0.numel() * p0.element_size()
            src, dst = torch.empty(moved // 2, dtype=torch.uint8, device=dev), torch.empty(moved // 2, dtype=torch.uint8, device=dev)
            ms = {"lmp_pack": [], "lmp_unpack": [], "copy": []}
            for it in range(warmup + calls):
                t = {}
                ctx.lightmap_pack_device(fmt, ch, texels, img.data_ptr(), p0.data_ptr())
                torch.cuda.synchronize()
                t["lmp_pack"] = ctx.last_kernel_ms()
                ctx.lightmap_unpack_device(fmt, ch, texels, p0.data_ptr(), u0.data_ptr())
                torch.cuda.synchronize()
                t["lmp_unpack"] = ctx.last_kernel_ms()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                t["copy"] = e0.elapsed_time(e1)
                if it >= warmup:
                    for key, val in t.items():
                        ms[key].append(val)
            del src, dst
            ctx.lightmap_pack_device(fmt, ch, made, mips.data_ptr(), pm.data_ptr())
            ctx.lightmap_unpack_device(fmt, ch, made, pm.data_ptr(), um.data_ptr())
            torch.cuda.synchronize()
            head = min(texels, 65536)
            host = img.reshape(-1, ch)[:head].cpu().numpy()
            want = lightmap_pack(host, fmt)
            got = p0[:want.size].cpu().numpy().view(want.dtype).reshape(want.shape)
            same = bool(np.array_equal(got, want) and np.array_equal(u0.reshape(-1, ch)[:head].cpu().numpy().view(np.int32),
                                                                     lightmap_unpack(want, fmt).view(np.int32)))
            copy = float(np.median(ms["copy"]))
            for key in ("lmp_pack", "lmp_unpack", "copy"):
                row = dict(mode="packed", size=size, format=name, query=key, calls=calls, bytes_moved=moved, **stats(ms[key]),
                           gb_per_s=round(moved / float(np.median(ms[key])) / 1e6, 1))
                if key != "copy":
                    row.update(over_copy=round(float(np.median(ms[key])) / copy, 4), equals_helper=same)
                emit(row)
            if not same:
                raise SystemExit("ray_query_bench: the packed texels differ from lightmap_pack / lightmap_unpack")
            stored[(fmt, ch)] = (p0, pm, u0, um, mv)
            del img, mips
        for n in point_counts:
            gw = 2 * size
            if n > gw * gw:
                raise SystemExit(f"ray_query_bench: {n} points exceed the {gw} x {gw} grid")

            def centres(k):                  # the uv of the points number k of the gw x gw grid, row-major
                u = ((k % gw).to(torch.float32) + 0.5) / gw
                v = 1.0 - ((k // gw).to(torch.float32) + 0.5) / gw
                return torch.stack([u, v], dim=1).contiguous()

            k = torch.arange(n, device=dev, dtype=torch.int64)
            anywhere = torch.randint(0, gw * gw, (n,), generator=gen, device=dev, dtype=torch.int64)
            nrm = torch.randn((n, 3), generator=gen, dtype=torch.float32, device=dev)
            nrm = (nrm / nrm.norm(dim=1, keepdim=True)).contiguous()
            lod = (torch.rand(n, generator=gen, dtype=torch.float32, device=dev) * 4.0).contiguous()
            w = torch.empty(n, dtype=torch.float32, device=dev)
            for order, uv in (("coherent", centres(k)), ("shuffled", centres(anywhere))):
                for with_lod in (True, False):
                    d, lv = (lod.data_ptr(), L) if with_lod else (None, 1)
                    pairs = {}
                    for (fmt, ch), (p0, pm, u0, um, mv) in stored.items():
                        m_p, m_u, m_v = (pm.data_ptr(), um.data_ptr(), mv.data_ptr()) if with_lod else (None, None, None)
                        out_p, out_f = torch.empty((n, ch), dtype=torch.float32, device=dev), torch.empty((n, ch), dtype=torch.float32, device=dev)
                        tag = ("f16" if fmt == F16 else "rgb9e5") + f"<{ch}>"
                        packed = (lambda fmt=fmt, ch=ch, p0=p0, m_p=m_p, m_v=m_v, o=out_p:
                                  ctx.lightmap_sample_packed_device(fmt, size, size, ch, p0.data_ptr(), lv, m_p, n, uv.data_ptr(), d, o.data_ptr(), w.data_ptr(),
                                                                    valid.data_ptr(), m_v))
                        if with_lod:
                            plain = (lambda ch=ch, u0=u0, m_u=m_u, m_v=m_v, o=out_f:
                                     ctx.lightmap_sample_lod_device(size, size, ch, u0.data_ptr(), L, m_u, n, uv.data_ptr(), d, o.data_ptr(), w.data_ptr(),
                                                                    valid.data_ptr(), m_v))
                        else:
                            plain = (lambda ch=ch, u0=u0, o=out_f:
                                     ctx.lightmap_sample_device(size, size, ch, u0.data_ptr(), n, uv.data_ptr(), o.data_ptr(), w.data_ptr(), valid.data_ptr()))
                        pairs["sample " + tag] = (packed, plain, out_p, out_f)
                    p0, pm, u0, um, mv = stored[(F16, 27)]
                    m_p, m_u, m_v = (pm.data_ptr(), um.data_ptr(), mv.data_ptr()) if with_lod else (None, None, None)
                    E_p, E_f = torch.empty((n, 3), dtype=torch.float32, device=dev), torch.empty((n, 3), dtype=torch.float32, device=dev)
                    packed = (lambda: ctx.lightmap_sh_sample_packed_device(F16, size, size, p0.data_ptr(), lv, m_p, n, uv.data_ptr(), nrm.data_ptr(), d,
                                                                           E_p.data_ptr(), w.data_ptr(), valid.data_ptr(), m_v))
                    if with_lod:
                        plain = (lambda: ctx.lightmap_sh_sample_lod_device(size, size, u0.data_ptr(), L, m_u, n, uv.data_ptr(), nrm.data_ptr(), d,
                                                                           E_f.data_ptr(), w.data_ptr(), valid.data_ptr(), m_v))
                    else:
                        plain = (lambda: ctx.lightmap_sh_sample_device(size, size, u0.data_ptr(), n, uv.data_ptr(), nrm.data_ptr(), E_f.data_ptr(), w.data_ptr(),
                                                                       valid.data_ptr()))
                    pairs["sh f16"] = (packed, plain, E_p, E_f)
                    ms = {key: ([], []) for key in pairs}
                    torch.cuda.synchronize()
                    for it in range(warmup + calls):
                        for key, (packed, plain, _, _) in pairs.items():
                            for side, call in enumerate((packed, plain)):
                                call()
                                torch.cuda.synchronize()
                                if it >= warmup:
                                    ms[key][side].append(ctx.last_kernel_ms())
                    for key, (_, _, out_p, out_f) in pairs.items():
                        same = same_bits(out_p, out_f)
                        base = dict(mode="packed", size=size, n_points=n, order=order, lod=with_lod, lookup=key, calls=calls)
                        emit(dict(base, query="f32", **stats(ms[key][1])))
                        emit(dict(base, query="packed", **stats(ms[key][0]),
                                  packed_over_f32=round(float(np.median(ms[key][0])) / float(np.median(ms[key][1])), 4), equals_f32_twin=same))
                        if not same:
                            raise SystemExit("ray_query_bench: a packed lookup differs from the f32 lookup of the unpacked texels")
                    del pairs, E_p, E_f
            del k, anywhere, nrm, lod, w
        del stored
    return rows


def bc6h_rows(ctx, sizes, point_counts, calls, warmup):
    """--mode bc6h: BC6H lightmaps on resident tables, HIP events inside the library (mi_last_kernel_ms), `warmup` calls then `calls` timed
    ones, medians with min - max; `spread` is (max - min) / median of a row.  Inputs per size: packed_rows' seeded random image
    [size, size, 3] in 0 .. 4 under its chart-and-gutter mask and its full mip chain.  Rows:
    "lmb_encode_block" (one lane per block, what ships) and "lmb_encode" (one lane per texel, MI_RT_LMB_LANE_PER_BLOCK=0, on a context of
    its own) of level 0 at rounds 0 and 2 and "lmb_decode", alternating with "lmp_pack rgb9e5" of the same image and with "copy", a
    device-to-device copy of the f32 bytes an encode reads (`over_copy`, `over_rgb9e5`: ratios of the medians); the blocks of the first
    64 block rows are checked against lightmap_bc6h_encode, the decoded texels against lightmap_bc6h_decode, bit for bit.
    Then, per point count and in lookup_rows' two orders, the BC6H lookup against its f32 twin (the f32 kernel on the texels
    mi_lightmap_bc6h_decode_device made of the same blocks) and against the RGB9E5 lookup of the same chain, with lod (uniform in 0 .. 4)
    and without; the BC6H and f32 outputs are compared on the device, every point, bit for bit.
    Quality: the cube of --mode adaptive baked in the Cornell box at 64 x 64 (64 samples), finished, under its own mask: the relative
    RMSE over valid texels of BC6H at rounds 0, 2 and 4 next to RGB9E5 and f16.  The measured figures are in DESIGN.md section 4,
    "BC6H lightmaps"."""
    from dataclasses import replace
    from cs397raytracingsp22_amd import (Lambertian, Scene, StaticMesh, abi, cgmath, lightmap_bc6h_decode, lightmap_bc6h_encode, lightmap_bc6h_layout,
                                         lightmap_mip_layout, lightmap_pack, lightmap_unpack, objload)
    dev = torch.device("cuda:0")
    RGB, F16 = abi.MI_LP_RGB9E5, abi.MI_LP_F16
    rows = []
    knob, before = "MI_RT_LMB_LANE_PER_BLOCK", os.environ.get("MI_RT_LMB_LANE_PER_BLOCK")
    os.environ[knob] = "0"                                         # read when a context is created: the one-lane-per-texel encoder
    try:
        per_texel = Context(0)
    finally:
        if before is None:
            del os.environ[knob]
        else:
            os.environ[knob] = before

    def stats(ms):
        med = float(np.median(ms))
        return {"ms_median": round(med, 4), "ms_min": round(float(np.min(ms)), 4), "ms_max": round(float(np.max(ms)), 4),
                "spread": round((float(np.max(ms)) - float(np.min(ms))) / med, 4)}

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    for size in sizes:
        layout, blocks_of = lightmap_mip_layout(size, size), lightmap_bc6h_layout(size, size)
        L, made, texels = len(layout), sum(w * h for w, h, _ in layout[1:]), size * size
        nb0, made_blocks = blocks_of[0][0] * blocks_of[0][1], sum(bw * bh for bw, bh, _ in blocks_of[1:])
        gen = torch.Generator(device=dev)
        gen.manual_seed(3)
        yy, xx = torch.meshgrid(torch.arange(size, device=dev), torch.arange(size, device=dev), indexing="ij")
        valid = ((xx % 64 < 60) & (yy % 64 < 60)).to(torch.uint8).contiguous()
        del yy, xx
        img = (torch.rand((size, size, 3), generator=gen, dtype=torch.float32, device=dev) * 4.0).contiguous()
        mips = torch.empty((made, 3), dtype=torch.float32, device=dev)
        mv = torch.empty(made, dtype=torch.uint8, device=dev)
        ctx.lightmap_mips_device(size, size, 3, img.data_ptr(), L, mips.data_ptr(), mv.data_ptr(), None, valid.data_ptr())
        b0 = torch.empty((nb0, 16), dtype=torch.uint8, device=dev)
        b1 = torch.empty((nb0, 16), dtype=torch.uint8, device=dev)
        bm = torch.empty((max(made_blocks, 1), 16), dtype=torch.uint8, device=dev)
        r0, rm = torch.empty(texels, dtype=torch.int32, device=dev), torch.empty(made, dtype=torch.int32, device=dev)
        u0, um = torch.empty_like(img), torch.empty_like(mips)
        src, dst = torch.empty(texels * 12, dtype=torch.uint8, device=dev), torch.empty(texels * 12, dtype=torch.uint8, device=dev)
        ms = {"lmb_encode_block rounds 0": [], "lmb_encode_block rounds 2": [], "lmb_encode rounds 0": [], "lmb_encode rounds 2": [], "lmb_decode": [],
              "lmp_pack rgb9e5": [], "copy": []}
        for it in range(warmup + calls):
            t = {}
            for rounds in (0, 2):
                ctx.lightmap_bc6h_encode_device(size, size, img.data_ptr(), b0.data_ptr(), rounds, valid.data_ptr())
                torch.cuda.synchronize()
                t[f"lmb_encode_block rounds {rounds}"] = ctx.last_kernel_ms()
                per_texel.lightmap_bc6h_encode_device(size, size, img.data_ptr(), b1.data_ptr(), rounds, valid.data_ptr())
                torch.cuda.synchronize()
                t[f"lmb_encode rounds {rounds}"] = per_texel.last_kernel_ms()
            ctx.lightmap_bc6h_decode_device(size, size, b0.data_ptr(), u0.data_ptr())
            torch.cuda.synchronize()
            t["lmb_decode"] = ctx.last_kernel_ms()
            ctx.lightmap_pack_device(RGB, 3, texels, img.data_ptr(), r0.data_ptr())
            torch.cuda.synchronize()
            t["lmp_pack rgb9e5"] = ctx.last_kernel_ms()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dst.copy_(src)
            e1.record()
            torch.cuda.synchronize()
            t["copy"] = e0.elapsed_time(e1)
            if it >= warmup:
                for key, val in t.items():
                    ms[key].append(val)
        del src, dst
        for l in range(1, L):                                      # the chain: one encode call per level, with its own mask
            (w, h, off), (bw, bh, boff) = layout[l], blocks_of[l]
            ctx.lightmap_bc6h_encode_device(w, h, mips.data_ptr() + off * 12, bm.data_ptr() + boff * 16, 2, mv.data_ptr() + off)
            ctx.lightmap_bc6h_decode_device(w, h, bm.data_ptr() + boff * 16, um.data_ptr() + off * 12)
        ctx.lightmap_pack_device(RGB, 3, made, mips.data_ptr(), rm.data_ptr())
        torch.cuda.synchronize()
        head = min(size, 256)                                      # texel rows checked on the host
        want = lightmap_bc6h_encode(img[:head].cpu().numpy(), valid[:head].cpu().numpy(), 2)
        got = b0[:want.shape[0] * want.shape[1]].cpu().numpy().reshape(want.shape)
        same = bool(np.array_equal(got, want) and torch.equal(b0, b1) and np.array_equal(u0[:head].cpu().numpy().view(np.int32), lightmap_bc6h_decode(want, size, head).view(np.int32)))
        copy, rgb = float(np.median(ms["copy"])), float(np.median(ms["lmp_pack rgb9e5"]))
        for key in ms:
            row = dict(mode="bc6h", size=size, query=key, calls=calls, **stats(ms[key]), mtexels_per_s=round(texels / float(np.median(ms[key])) / 1e3, 1))
            if key.startswith("lmb"):
                row.update(over_copy=round(float(np.median(ms[key])) / copy, 3), over_rgb9e5=round(float(np.median(ms[key])) / rgb, 3), equals_helper=same)
            emit(row)
        if not same:
            raise SystemExit("ray_query_bench: the blocks differ from lightmap_bc6h_encode / lightmap_bc6h_decode")
        for n in point_counts:
            gw = 2 * size
            if n > gw * gw:
                raise SystemExit(f"ray_query_bench: {n} points exceed the {gw} x {gw} grid")

            def centres(k):                  # the uv of the points number k of the gw x gw grid, row-major
                u = ((k % gw).to(torch.float32) + 0.5) / gw
                v = 1.0 - ((k // gw).to(torch.float32) + 0.5) / gw
                return torch.stack([u, v], dim=1).contiguous()

            k = torch.arange(n, device=dev, dtype=torch.int64)
            anywhere = torch.randint(0, gw * gw, (n,), generator=gen, device=dev, dtype=torch.int64)
            lod = (torch.rand(n, generator=gen, dtype=torch.float32, device=dev) * 4.0).contiguous()
            w = torch.empty(n, dtype=torch.float32, device=dev)
            outs = {key: torch.empty((n, 3), dtype=torch.float32, device=dev) for key in ("bc6h", "f32", "rgb9e5")}
            for order, uv in (("coherent", centres(k)), ("shuffled", centres(anywhere))):
                for with_lod in (True, False):
                    d, lv = (lod.data_ptr(), L) if with_lod else (None, 1)
                    m_b, m_u, m_r, m_v = (bm.data_ptr(), um.data_ptr(), rm.data_ptr(), mv.data_ptr()) if with_lod else (None, None, None, None)
                    call = {
                        "bc6h": lambda: ctx.lightmap_sample_bc6h_device(size, size, b0.data_ptr(), lv, m_b, n, uv.data_ptr(), d, outs["bc6h"].data_ptr(),
                                                                        w.data_ptr(), valid.data_ptr(), m_v),
                        "rgb9e5": lambda: ctx.lightmap_sample_packed_device(RGB, size, size, 3, r0.data_ptr(), lv, m_r, n, uv.data_ptr(), d,
                                                                            outs["rgb9e5"].data_ptr(), w.data_ptr(), valid.data_ptr(), m_v),
                        "f32": (lambda: ctx.lightmap_sample_lod_device(size, size, 3, u0.data_ptr(), L, m_u, n, uv.data_ptr(), d, outs["f32"].data_ptr(),
                                                                       w.data_ptr(), valid.data_ptr(), m_v)) if with_lod else
                               (lambda: ctx.lightmap_sample_device(size, size, 3, u0.data_ptr(), n, uv.data_ptr(), outs["f32"].data_ptr(), w.data_ptr(),
                                                                   valid.data_ptr())),
                    }
                    took = {key: [] for key in call}
                    torch.cuda.synchronize()
                    for it in range(warmup + calls):
                        for key, fn in call.items():
                            fn()
                            torch.cuda.synchronize()
                            if it >= warmup:
                                took[key].append(ctx.last_kernel_ms())
                    same = bool(torch.equal(outs["bc6h"].view(torch.int32), outs["f32"].view(torch.int32)))
                    f32_ms = float(np.median(took["f32"]))
                    for key in call:
                        row = dict(mode="bc6h", size=size, n_points=n, order=order, lod=with_lod, query=key, calls=calls, **stats(took[key]),
                                   over_f32=round(float(np.median(took[key])) / f32_ms, 4))
                        if key == "bc6h":
                            row.update(equals_f32_twin=same)
                        emit(row)
                    if not same:
                        raise SystemExit("ray_query_bench: a BC6H lookup differs from the f32 lookup of the decoded texels")
            del k, anywhere, lod, w, outs
        del img, mips, b0, bm, r0, rm, u0, um
    # quality: the finished cube bake under its own mask
    import gzip
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with gzip.open(os.path.join(root, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
        cube = objload.load_obj_text(fh.read())[0]
    xf = cgmath.mul(cgmath.from_translation((0.2, 1.6, -0.3)), cgmath.from_angle_y(25.0), cgmath.from_scale(0.8))
    box = StaticMesh(cube, Lambertian(albedo=(0.7, 0.7, 0.7)), [None] * 5, xf)
    sc = Scene(replace(scenes.config4(64, 64, 64, 10).camera, path_depth=6), scenes.cornell_walls() + [box])
    ctx.upload(sc.flatten())
    mean = ctx.bake_lightmap_sh(replace(sc.camera, screen_width=64, screen_height=64, aa_sample_count=64), box, jitter=True, offset=1e-3, seed=5)[1]
    p1, n1, _ = ctx.lightmap_texels(box, 64, 64, rows=1, offset=1e-3)
    fin, ok = ctx.lightmap_finish(mean, p1[0], n1[0], levels=1, dilate=2)
    keep = ok != 0
    ref = fin.astype(np.float64)[keep]

    def rel_rmse(x):
        return float(np.sqrt(((x.astype(np.float64)[keep] - ref) ** 2).sum() / (ref ** 2).sum()))

    quality = {f"bc6h rounds {r}": rel_rmse(ctx.lightmap_bc6h_decode(ctx.lightmap_bc6h_encode(fin, ok, r), 64, 64)) for r in (0, 2, 4)}
    quality["rgb9e5"] = rel_rmse(lightmap_unpack(lightmap_pack(fin, RGB), RGB))
    quality["f16"] = rel_rmse(lightmap_unpack(lightmap_pack(fin, F16), F16))
    per_texel.close()
    for key, val in quality.items():
        emit(dict(mode="bc6h", query="quality", image="cube bake 64 x 64, finished", valid_texels=int(keep.sum()), format=key, rel_rmse=float(f"{val:.4g}")))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20, help="timed calls per row (at least 20)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--mode", choices=("intersect", "occlusion", "render", "hemisphere", "bake", "probes", "atlas", "finish", "volume", "variance", "adaptive", "directional", "lookup", "mips", "packed", "bc6h"), default="intersect",
                    help="intersect: the closest-hit rows; occlusion: the any-hit query against the visibility form; "
                         "render: ray-table rendering against mi_shade_rays_device; "
                         "hemisphere: hemisphere occlusion against the any-hit query on the identical pre-made rays; "
                         "bake: point-table rendering against ray-table rendering on the identical pre-made rays; "
                         "probes: light-probe rendering against ray-table rendering on the identical pre-made rays; "
                         "atlas: the lightmap atlas on the GPU against the host helper, on the drone; "
                         "finish: lightmap finishing pass by pass, both forms of the filter, against a copy of the same bytes; "
                         "volume: irradiance-volume sampling, coherent and shuffled points, against a copy of the same bytes; "
                         "variance: the bake's second moments against the plain bake, the variance-guided finish against the fixed one; "
                         "adaptive: the adaptive bake against uniform bakes at the same and at the largest sample count, errors against a "
                         "16 x reference, and the bookkeeping kernels' share of a round; "
                         "directional: wf_reduce_psh's share of an SH bake, the 27-channel finish against nine 3-channel ones, and the "
                         "evaluation against a copy of the same bytes; "
                         "lookup: the lightmap lookup kernels, coherent and shuffled uv, the fused SH form against lml_sample<27> + lsh_eval "
                         "and against a copy of the same bytes; "
                         "mips: the lightmap mip chain, five levels per launch against one, against a copy of the nominal bytes, and the "
                         "trilinear lookups against the level-0 lookups on the same points; "
                         "packed: lmp_pack / lmp_unpack against a copy of the same bytes, and every packed lookup against its f32 twin; "
                         "bc6h: the BC6H encoder and decoder against a copy and RGB9E5, the BC6H lookup against the f32 and RGB9E5 ones, quality")
    ap.add_argument("--lookup-sizes", default="1024,2048", help="--mode lookup, --mode mips and --mode packed: the square lightmap sizes")
    ap.add_argument("--volume-grids", default="16,32", help="--mode volume: probes per axis")
    ap.add_argument("--volume-points", default=f"{1 << 20},{1 << 22}", help="--mode volume, --mode directional, --mode lookup, --mode mips and --mode packed: point counts")
    ap.add_argument("--finish-sizes", default="1024,2048,4096", help="--mode finish and --mode variance: the square atlas sizes")
    ap.add_argument("--atlas-sizes", default="1024,2048", help="--mode atlas: the square atlas sizes")
    ap.add_argument("--atlas-grid", type=int, default=0, help="--mode atlas: a synthetic height field of N x N quads (2 N^2 triangles) instead "
                    "of the drone; the table's timings and the check against the helper only, no bake")
    ap.add_argument("--atlas-bakes", type=int, default=3, help="--mode atlas: timed whole bakes per size and side (after one warm-up)")
    ap.add_argument("--points", type=int, default=1 << 18, help="--mode hemisphere: at most this many surface points (64 rays each)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if not torch.cuda.is_available():
        raise SystemExit("ray_query_bench: no GPU; there is no CPU fallback")
    rows = []
    if a.mode == "finish":
        for size in [int(v) for v in a.finish_sizes.split(",")]:
            rows += finish_rows(size, a.calls, a.warmup)
        a.configs = ""
    ctx = Context(0)
    if a.mode == "volume":
        rows += volume_rows(ctx, [int(v) for v in a.volume_grids.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "variance":
        rows += variance_rows(ctx, [int(v) for v in a.finish_sizes.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "directional":
        rows += directional_rows(ctx, [int(v) for v in a.finish_sizes.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "lookup":
        rows += lookup_rows(ctx, [int(v) for v in a.lookup_sizes.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "mips":
        rows += mips_rows(ctx, [int(v) for v in a.lookup_sizes.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "packed":
        rows += packed_rows(ctx, [int(v) for v in a.lookup_sizes.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "bc6h":
        rows += bc6h_rows(ctx, [int(v) for v in a.lookup_sizes.split(",")], [int(v) for v in a.volume_points.split(",")], a.calls, a.warmup)
        a.configs = ""
    if a.mode == "adaptive":
        rows += adaptive_rows(ctx, int(a.atlas_sizes.split(",")[0]), a.atlas_bakes)
        a.configs = ""
    if a.mode == "atlas":
        for size in [int(v) for v in a.atlas_sizes.split(",")]:
            rows += atlas_rows(ctx, size, a.calls, a.warmup, a.atlas_bakes, a.atlas_grid)
        a.configs = ""
    for cfg in [int(c) for c in a.configs.split(",") if c]:
        sc = {2: scenes.config2, 4: scenes.config4}[cfg](a.width, a.height, 1, 10)
        ctx.upload(sc.flatten())
        co, cd = pinhole_rays(sc.camera)
        if a.mode == "probes":
            rows += probes_rows(ctx, cfg, sc, a.calls, a.warmup)
            continue
        if a.mode == "render":
            rows += render_rows(ctx, cfg, sc, co, cd, a.calls, a.warmup)
            continue
        first = ctx.intersect_rays(co, cd, t_max=sc.camera.max_trace_dist)
        if a.mode == "bake":
            rows += bake_rows(ctx, cfg, sc, first, a.calls, a.warmup)
            continue
        hit = first.object >= 0
        rng = np.random.default_rng(1)
        bd = rng.standard_normal((int(hit.sum()), 3))
        bd = np.ascontiguousarray(bd / np.linalg.norm(bd, axis=1, keepdims=True), np.float32)
        bo = np.ascontiguousarray(first.hitpoint[hit])
        if a.mode == "hemisphere":
            ok = np.flatnonzero(hit & np.any(first.normal != 0.0, axis=1))
            ok = ok[np.linspace(0, len(ok) - 1, min(len(ok), a.points)).astype(np.int64)]
            rows += hemisphere_rows(ctx, cfg, np.ascontiguousarray(first.hitpoint[ok]), np.ascontiguousarray(first.normal[ok]),
                                    a.calls, a.warmup)
            continue
        if a.mode == "occlusion":
            rows += occlusion_rows(ctx, cfg, sc, co, cd, bo, bd, np.ascontiguousarray(first.hitpoint[hit]), a.calls, a.warmup)
            continue
        for set_name, o, d, t_max in (("camera", co, cd, sc.camera.max_trace_dist), ("bounce", bo, bd, float("inf"))):
            for resolve in (True, False):
                med, wall, lo, hi, hits = measure(ctx, o, d, t_max, resolve, a.calls, a.warmup)
                row = {"config": cfg, "rays": set_name, "resolve": resolve, "n_rays": len(o), "hits": hits, "calls": a.calls,
                       "kernel_ms_median": round(med, 4), "kernel_ms_min": round(lo, 4), "kernel_ms_max": round(hi, 4),
                       "wall_ms_median": round(wall, 4), "mrays_per_s_kernel": round(len(o) / med / 1e3, 1),
                       "mrays_per_s_wall": round(len(o) / wall / 1e3, 1)}
                rows.append(row)
                print(json.dumps(row), flush=True)
    ctx.close()
    if a.out:
        with open(a.out, "a") as fh:
            for row in rows:
                fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
