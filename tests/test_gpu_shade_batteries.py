"""The shading batteries of tests/shade_batteries.py through mi_shade_rays — HIP through the C ABI against the oracle's orc_shade, ray by
ray, every call of every battery: the radiance is equal as f32 values, NaN exactly where the oracle has NaN (same_f32).  Ray i of a call
is keyed (seed, first_key + i, 0) on both sides; a call sets path_depth, path_samples and max_trace_dist.  The batteries with a StaticMesh
probe run once more in a context created under MI_RT_GLOBAL_BVH=1; one battery goes through mi_shade_rays_device and one is split into two
half batches.

What each battery's census holds, that a mutated oracle is noticed, and the float64 check of the oracle's estimator are on the CPU
(tests/test_shade_batteries_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from cs397raytracingsp22_amd import Camera, Context, abi

import shade_batteries as sb
from test_gpu_ray_queries import same_f32

pytestmark = pytest.mark.gpu

SEED = sb.SEED


@pytest.fixture(scope="module")
def global_ctx():
    os.environ["MI_RT_GLOBAL_BVH"] = "1"
    try:
        ctx = Context(0)
    finally:
        del os.environ["MI_RT_GLOBAL_BVH"]
    yield ctx
    ctx.close()


def oracle_shades(osc, cam, o, d, key):
    return np.stack([osc.shade(cam, o[i], d[i], seed=SEED, pixel=key + i, sample=0) for i in range(len(o))])


def run_battery(ctx, orc, label, bat):
    """Every call of the battery against the oracle.  Prints, per battery, the rays, the differing components and the (call, ray) pairs the
    census puts on an edge; returns (differing components, components, description of the first differing call)."""
    sc, cam, o, d, calls, census = bat
    flat = sc.flatten()
    ctx.upload(flat)
    osc = orc.OracleScene(flat)
    bad_total, n_total, first = 0, 0, None
    purpose = np.broadcast_to(census["purpose"], (len(calls), len(o)))
    for ci, (key, depth, samples, tmax) in enumerate(calls):
        cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
        ref = oracle_shades(osc, cam, o, d, key)
        got = ctx.shade_rays(cam, o, d, seed=SEED, first_key=key)
        bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
        assert same_f32(got, ref) == (not bad.any())
        if bad.any() and first is None:
            i = int(np.flatnonzero(bad.any(axis=1))[0])
            first = (label, (key, depth, samples, tmax), i, o[i].tolist(), d[i].tolist(), got[i].tolist(), ref[i].tolist())
        bad_total += int(bad.sum())
        n_total += bad.size
    osc.close()
    print(f"{label}: {len(o)} rays x {len(calls)} calls, {bad_total} of {n_total} components differ, {int(purpose.sum())} (call, ray) pairs on an edge on purpose")
    return bad_total, n_total, first


@pytest.mark.parametrize("family", sb.FAMILIES)
def test_shade_battery(gpu_ctx, orc, family):
    results = [run_battery(gpu_ctx, orc, label, bat) for label, bat in sb.all_batteries(family)]
    assert len(results) >= 1 and all(n > 0 for _, n, _ in results)
    firsts = [f for _, _, f in results if f is not None]
    assert sum(b for b, _, _ in results) == 0, firsts[:4]


def test_mesh_probe_batteries_global_bvh(global_ctx, orc):
    """The StaticMesh probes once more with the tree read from global memory."""
    done = []
    for family in ("critical", "lobe_kinds", "dot_term"):
        for label, bat in sb.all_batteries(family):
            if label in sb.MESH_PROBE_LABELS:
                done.append(run_battery(global_ctx, orc, label + " (global tree)", bat))
    assert len(done) == len(sb.MESH_PROBE_LABELS)
    assert sum(b for b, _, _ in done) == 0, [f for _, _, f in done if f is not None][:4]


def test_device_form_equals_the_host_form(gpu_ctx):
    import torch
    sc, cam, o, d, calls, _ = sb.lobe_battery(1.0, 0.5, "plane")
    gpu_ctx.upload(sc.flatten())
    dev = torch.device("cuda:0")
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    for key, depth, samples, tmax in calls[:6] + [(5, 6, 3, 100.0)]:
        cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
        host = gpu_ctx.shade_rays(cam, o, d, seed=SEED, first_key=key)
        t_rgb = torch.full((len(o), 3), -7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        gpu_ctx.shade_rays_device(cam, len(o), t_o.data_ptr(), t_d.data_ptr(), t_rgb.data_ptr(), seed=SEED, first_key=key)
        torch.cuda.synchronize()
        assert t_rgb.cpu().numpy().tobytes() == host.tobytes(), (key, depth, samples)
        assert host.any()


def test_two_half_batches_give_the_same_bytes(gpu_ctx):
    sc, cam, o, d, calls, _ = sb.depth_battery()
    gpu_ctx.upload(sc.flatten())
    h = 100                                                                       # not a multiple of the wave
    for key, depth, samples, tmax in calls:
        cam.path_depth, cam.path_samples, cam.max_trace_dist = depth, samples, tmax
        one = gpu_ctx.shade_rays(cam, o, d, seed=SEED, first_key=key)
        two = np.concatenate([gpu_ctx.shade_rays(cam, o[:h], d[:h], seed=SEED, first_key=key),
                              gpu_ctx.shade_rays(cam, o[h:], d[h:], seed=SEED, first_key=key + h)])
        assert one.tobytes() == two.tobytes(), (key, depth, samples, tmax)
    sc, cam, o, d, calls, _ = sb.dot_term_battery("metal2")                       # every ray draws: the keys matter
    gpu_ctx.upload(sc.flatten())
    cam.path_depth, cam.path_samples, cam.max_trace_dist = 4, 2, sb.INF
    one = gpu_ctx.shade_rays(cam, o, d, seed=SEED, first_key=40)
    two = np.concatenate([gpu_ctx.shade_rays(cam, o[:h], d[:h], seed=SEED, first_key=40), gpu_ctx.shade_rays(cam, o[h:], d[h:], seed=SEED, first_key=40 + h)])
    assert one.tobytes() == two.tobytes()
    other = gpu_ctx.shade_rays(cam, o, d, seed=SEED, first_key=41)
    assert other.tobytes() != one.tobytes()


def test_shade_rays_refuses_zero_path_samples_and_a_nan_max_trace_dist(gpu_ctx, orc):
    """mi_render's refusals (render_plan.cpp), which mi_shade_rays lacked: path_samples == 0 gave emission + 0 / 0.  The oracle's
    check_camera refuses path_samples == 0 too.  The check stands before the have_scene test."""
    lib = abi.load()
    sc, cam, o, d, calls, _ = sb.depth_battery()
    flat = sc.flatten()
    gpu_ctx.upload(flat)
    import torch
    rgb = np.full((len(o), 3), -9.0, np.float32)
    po, pd, prgb = o.ctypes.data, d.ctypes.data, rgb.ctypes.data
    dev = torch.device("cuda:0")                                                  # the _device form gets device buffers: a check that regressed must not fault
    t_o, t_d = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    t_rgb = torch.full((len(o), 3), -9.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    fresh = Context(0)                                                            # no scene uploaded
    try:
        for h in (gpu_ctx._h, fresh._h):
            for field, value, words in (("path_samples", 0, b"path_samples must be >= 1"), ("max_trace_dist", float("nan"), b"max_trace_dist must not be NaN")):
                pod = Camera(path_depth=2).to_pod()
                setattr(pod, field, value)
                assert lib.mi_shade_rays(h, C.byref(pod), len(o), po, pd, SEED, 0, prgb) == abi.MI_ERR_INVALID, field
                assert words in lib.mi_last_error(), (field, lib.mi_last_error())
                assert lib.mi_shade_rays_device(h, C.byref(pod), len(o), t_o.data_ptr(), t_d.data_ptr(), SEED, 0, t_rgb.data_ptr(), None) == abi.MI_ERR_INVALID, field
                assert lib.mi_shade_rays(h, C.byref(pod), 0, po, pd, SEED, 0, prgb) == abi.MI_ERR_INVALID, field      # even for no rays
        ok = Camera(path_depth=2).to_pod()
        assert lib.mi_shade_rays(fresh._h, C.byref(ok), len(o), po, pd, SEED, 0, prgb) == abi.MI_ERR_NO_SCENE
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert np.all(rgb == -9.0) and bool((t_rgb == -9.0).all())                    # nothing was written
    pod = Camera(path_depth=2, max_trace_dist=float("inf")).to_pod()              # +inf stays legal
    assert lib.mi_shade_rays(gpu_ctx._h, C.byref(pod), len(o), po, pd, SEED, 0, prgb) == abi.MI_OK and np.isfinite(rgb).all()
    for bad in (Camera(path_samples=0), Camera(max_trace_dist=float("nan"))):     # the Python wrapper refuses before the library is called
        with pytest.raises(ValueError):
            gpu_ctx.shade_rays(bad, o, d, seed=SEED)
    osc = orc.OracleScene(flat)
    with pytest.raises(RuntimeError):
        osc.shade(Camera(path_samples=0), o[0], d[0], seed=SEED)
    osc.close()
