"""Occlusion queries — mi_occluded_rays / mi_occluded_rays_device, the any-hit kernel rq_occluded — HIP through the C ABI.

occluded[i] must be true exactly when Scene::intersect_ray(ray_i, t_min, t_max_i) (tracing.rs:326-346) returns Some.  Every comparison
here is equality of booleans, ray by ray, every ray.  The reference is the oracle: `oracle_hits(...)["object"] >= 0` for a scalar
interval, `OracleScene.intersect(..., t_max=ray_t_max[i]).hit` called per ray for per-ray intervals; the consistency tests compare with
the library's own closest-hit query in its visibility form instead.  Ray i of a call is keyed (seed, first_key + i, 0) on both sides.

Rays per named scene: 1024 camera rays (the oracle's generate_rays at seeded random pixels), one bounce ray per camera hit, 96 hand-made
edge rays in three calls — the sets and intervals of tests/test_gpu_ray_queries.py check_scene — then per-ray t_max at, half of, one ulp
below and one ulp above the oracle's closest distance, and segments from every camera hitpoint to two fixed points."""
import numpy as np
import pytest

from cs397raytracingsp22_amd import Context, Triangle, abi, scenes

import ray_batteries as rb
from test_gpu_ray_batteries import global_ctx                                   # noqa: F401  (fixture: a context under MI_RT_GLOBAL_BVH=1)
from test_gpu_ray_queries import (INF, NAMED, OTHER, SEED, bounce_rays, camera_rays, edge_rays, long_triangle_list, oracle_hits,
                                  some_rays)

pytestmark = pytest.mark.gpu

N_CAM = 1024
F = np.float32


# ---------------------------------------------------------------- the oracle's side (no GPU in here)
def scene_case(orc, sc):
    """The ray sets of check_scene with the oracle's answers: a list of (what, o, d, t_min, t_max, first_key, ref occluded), plus the
    camera rays' full oracle records."""
    flat = sc.flatten()
    osc = orc.OracleScene(flat)
    kinds = np.array([flat.desc.objects[k].kind for k in range(flat.desc.n_objects)])
    rng = np.random.default_rng(1)
    calls = []

    def add(what, o, d, t_min, t_max, key):
        assert np.isfinite(o).all() and np.isfinite(d).all() and np.all(np.any(d != 0.0, axis=1)), what
        ref = oracle_hits(osc, o, d, t_min, t_max, SEED, key)
        calls.append((what, o, d, t_min, t_max, key, ref["object"] >= 0))
        return ref

    co, cd = camera_rays(orc, sc.camera, N_CAM, rng)
    ref_cam = add("camera", co, cd, 0.001, sc.camera.max_trace_dist, 0)
    bo, bd = bounce_rays(ref_cam, rng)
    if len(bo):
        add("bounce", bo, bd, 0.001, INF, N_CAM)
    eo, ed = edge_rays(sc, ref_cam, kinds, rng)
    add("edge axis", eo, ed, 0.001, INF, 100000)
    add("edge t_min=0", eo, ed, 0.0, INF, 200000)
    dist = ref_cam["distance"][ref_cam["object"] >= 0]
    short = float(np.median(dist)) * 0.5 if len(dist) else 1.0
    add("edge short t_max", np.concatenate([co[:48], eo[:48]]), np.concatenate([cd[:48], ed[:48]]), 0.001, short, 300000)
    osc.close()
    return {"sc": sc, "flat": flat, "calls": calls, "co": co, "cd": cd, "ref_cam": ref_cam}


_NAMED_CASES = {}


def named_case(orc, name):
    """Computed once per named scene and shared by the tests below; nothing in it is modified afterwards."""
    if name not in _NAMED_CASES:
        case = scene_case(orc, NAMED[name]())
        for _, o, d, _, _, _, ref in case["calls"]:
            for a in (o, d, ref):
                a.flags.writeable = False
        _NAMED_CASES[name] = case
    return _NAMED_CASES[name]


def oracle_occluded_per_ray(osc, o, d, t_min, ray_t_max, first_key):
    return np.array([bool(osc.intersect(o[i], d[i], t_min=t_min, t_max=float(ray_t_max[i]), seed=SEED, pixel=first_key + i, sample=0).hit)
                     for i in range(len(o))], bool)


FLAVOURS = ("0.5 D", "D", "one ulp below D", "one ulp above D")


def flavour_case(orc, name, first_key=500000):
    """The camera rays the oracle hits, four times over, with ray_t_max = 0.5 D | D | nextafter(D, 0) | nextafter(D, +inf) of the
    oracle's closest distance D, and the oracle's answer for each (called per ray with that ray's t_max)."""
    case = named_case(orc, name)
    ref = case["ref_cam"]
    hit = np.flatnonzero(ref["object"] >= 0)
    D = ref["distance"][hit].astype(F)
    tm = np.concatenate([F(0.5) * D, D, np.nextafter(D, F(0.0)), np.nextafter(D, F(INF))]).astype(F)
    o, d = np.tile(case["co"][hit], (4, 1)), np.tile(case["cd"][hit], (4, 1))
    osc = orc.OracleScene(case["flat"])
    want = oracle_occluded_per_ray(osc, o, d, 0.001, tm, first_key)
    osc.close()
    return o, d, tm, first_key, want, len(hit)


def segment_case(orc, name, first_key=600000):
    """From every camera hitpoint p to L1 = (0, 4.5, 0) and to L2 = eye + (1.5, 1.0, -2.0), all in f32: o = p, d = L - p, [0.001, 0.999]."""
    case = named_case(orc, name)
    ref = case["ref_cam"]
    p = ref["hitpoint"][ref["object"] >= 0].astype(F)
    eye = np.array(case["sc"].camera.eyepoint, F)
    L1, L2 = np.array([0.0, 4.5, 0.0], F), (eye + np.array([1.5, 1.0, -2.0], F)).astype(F)
    o = np.concatenate([p, p])
    d = np.concatenate([(L1 - p).astype(F), (L2 - p).astype(F)])
    keep = np.any(d != 0.0, axis=1)                                             # a hitpoint that IS the point has no segment
    o, d = np.ascontiguousarray(o[keep]), np.ascontiguousarray(d[keep])
    osc = orc.OracleScene(case["flat"])
    want = oracle_hits(osc, o, d, 0.001, 0.999, SEED, first_key)["object"] >= 0
    osc.close()
    return o, d, first_key, want


def assert_same(got, want, what):
    assert got.dtype == bool and got.shape == want.shape, what
    bad = np.flatnonzero(got != want)
    print(f"{what}: {len(want)} rays, oracle true {int(want.sum())}, mismatches {len(bad)}")
    assert len(bad) == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


# ---------------------------------------------------------------- 1. scalar interval against the oracle
def run_scene_case(ctx, case, name):
    ctx.upload(case["flat"])
    for what, o, d, t_min, t_max, key, want in case["calls"]:
        got = ctx.occluded_rays(o, d, t_min=t_min, t_max=t_max, seed=SEED, first_key=key)
        assert_same(got, want, f"{name} {what}")


@pytest.mark.parametrize("name", sorted(NAMED))
def test_occluded_matches_the_oracle_named_scenes(gpu_ctx, orc, name):
    case = named_case(orc, name)
    run_scene_case(gpu_ctx, case, name)
    both = np.concatenate([c[6] for c in case["calls"] if c[0] in ("camera", "bounce")])
    share = float(both.mean())
    print(f"{name}: oracle's occluded share over camera + bounce rays {share:.3f}")
    assert 0.25 <= share <= 0.75, share                                        # not vacuous: the bar check_scene asserts


@pytest.mark.parametrize("name", sorted(OTHER))
def test_occluded_matches_the_oracle_other_scenes(gpu_ctx, orc, name):
    sc = OTHER[name]()
    if name == "long_list":
        assert sum(isinstance(o, Triangle) for o in sc.objects) >= 105         # the top-level tree's any-hit form is walked
    run_scene_case(gpu_ctx, scene_case(orc, sc), name)


# ---------------------------------------------------------------- 2. per-ray t_max against the oracle called per ray
@pytest.mark.parametrize("name", sorted(NAMED))
def test_per_ray_t_max_matches_the_oracle(gpu_ctx, orc, name):
    o, d, tm, key, want, n = flavour_case(orc, name)
    gpu_ctx.upload(named_case(orc, name)["flat"])
    got = gpu_ctx.occluded_rays(o, d, t_min=0.001, t_max=12345.0, ray_t_max=tm, seed=SEED, first_key=key)     # the scalar is replaced
    for k, fl in enumerate(FLAVOURS):
        print(f"{name} t_max = {fl}: oracle true {int(want[k * n:(k + 1) * n].sum())} of {n}")
    assert_same(got, want, f"{name} per-ray t_max")
    share = float(want.mean())
    assert 0.25 <= share <= 0.75, share
    at_d, below = want[n:2 * n], want[2 * n:3 * n]
    assert (at_d & ~below).any()                                                # some ray is true at D and false one ulp below


# ---------------------------------------------------------------- 3. segments
@pytest.mark.parametrize("name", sorted(NAMED))
def test_segments_to_two_points_match_the_oracle(gpu_ctx, orc, name):
    o, d, key, want = segment_case(orc, name)
    gpu_ctx.upload(named_case(orc, name)["flat"])
    got = gpu_ctx.occluded_rays(o, d, t_min=0.001, t_max=0.999, seed=SEED, first_key=key)
    assert_same(got, want, f"{name} segments")
    assert int(want.sum()) >= 32 and int((~want).sum()) >= 32, (int(want.sum()), int((~want).sum()))


# ---------------------------------------------------------------- 4. consistency with the closest-hit query
def consistent(ctx, what, battery):
    """Every call of the battery: occluded == (the visibility form's object >= 0).  Returns how many rays are occluded."""
    sc, o, d, calls, _ = battery
    ctx.upload(sc.flatten())
    total = 0
    for t_min, t_max, key in calls:
        occ = ctx.occluded_rays(o, d, t_min=t_min, t_max=t_max, seed=SEED, first_key=key)
        vis = ctx.intersect_rays(o, d, t_min=t_min, t_max=t_max, seed=SEED, first_key=key, resolve=False)
        bad = np.flatnonzero(occ != (vis.object >= 0))
        assert len(bad) == 0, (what, (t_min, t_max), bad[:8], vis.object[bad[:8]])
        total += int(occ.sum())
    print(f"{what}: {len(calls)} calls of {len(o)} rays, {total} occluded")
    return total


@pytest.mark.parametrize("which", ["sphere", "triangle", "plane", "window", "magnitude", "volume"])
def test_batteries_agree_with_the_closest_hit_query(gpu_ctx, which):
    assert consistent(gpu_ctx, which, getattr(rb, which + "_battery")()) > 0


@pytest.mark.parametrize("ctx_kind", ["lds", "global"])
@pytest.mark.parametrize("transform", sorted(rb.MESH_TRANSFORMS))
def test_mesh_battery_agrees_with_the_closest_hit_query(gpu_ctx, global_ctx, transform, ctx_kind):     # noqa: F811
    ctx = gpu_ctx if ctx_kind == "lds" else global_ctx
    assert consistent(ctx, f"mesh {transform} {ctx_kind}", rb.mesh_battery(transform)) > 0


@pytest.mark.parametrize("ctx_kind", ["lds", "global"])
def test_texture_battery_agrees_with_the_closest_hit_query(gpu_ctx, global_ctx, ctx_kind):              # noqa: F811
    ctx = gpu_ctx if ctx_kind == "lds" else global_ctx
    for size in rb.TEX_SIZES:
        for uvs in sorted(rb.QUAD_UVS):
            assert consistent(ctx, f"texture {size} {uvs} {ctx_kind}", rb.texture_battery(size, uvs)) >= 20


def test_long_list_battery_agrees_with_the_closest_hit_query(gpu_ctx):
    sc = long_triangle_list()
    assert sum(isinstance(o, Triangle) for o in sc.objects) >= 105             # long enough for the top-level tree (>= 96 small ones)
    assert consistent(gpu_ctx, "long list", rb.long_list_battery(sc)) > 0


@pytest.mark.parametrize("kind", ["spheres", "triangles", "planes", "mesh", "mixed"])
def test_nonfinite_battery_agrees_with_the_closest_hit_query(gpu_ctx, kind):
    """`best_hit` never goes back to None, so the OR over the objects is order-free even at NaN distances: exact here too."""
    assert consistent(gpu_ctx, f"non-finite {kind}", rb.nonfinite_battery(kind)) > 0


# ---------------------------------------------------------------- 5. entry points
def volume_rays(orc, name):
    """Camera rays (t_max = inf) and their bounces with t_max = 0.5: the media measure their free path in units of the parameter
    (geometry.rs:517 against t_end - t_start), so over [0.001, 0.5] a bounce that starts inside a medium scatters or not by its draw,
    and a short direction keeps everything else out of the interval."""
    case = named_case(orc, name)
    calls = {c[0]: c for c in case["calls"]}
    o = np.concatenate([calls["camera"][1], calls["bounce"][1]])
    d = np.concatenate([calls["camera"][2], calls["bounce"][2]])
    tm = np.full(len(o), 0.5, F)
    tm[:N_CAM] = F(INF)
    return o, d, tm


@pytest.mark.parametrize("name", ["config5", "head_scene"])
def test_two_half_batches_equal_one_batch(gpu_ctx, orc, name):
    o, d, tm = volume_rays(orc, name)
    gpu_ctx.upload(named_case(orc, name)["flat"])
    one = gpu_ctx.occluded_rays(o, d, ray_t_max=tm, seed=SEED, first_key=40)
    h = 1100
    a = gpu_ctx.occluded_rays(o[:h], d[:h], ray_t_max=tm[:h], seed=SEED, first_key=40)
    b = gpu_ctx.occluded_rays(o[h:], d[h:], ray_t_max=tm[h:], seed=SEED, first_key=40 + h)
    assert np.array_equal(np.concatenate([a, b]), one)
    stale = gpu_ctx.occluded_rays(o[h:], d[h:], ray_t_max=tm[h:], seed=SEED, first_key=40)
    print(f"{name}: {int(one.sum())} of {len(one)} occluded; {int((stale != one[h:]).sum())} answers move when first_key is not advanced")
    assert (stale != one[h:]).any()                                             # the stream is observable: the keying matters


def test_host_and_device_entry_points_agree(gpu_ctx, orc):
    import torch
    o, d, tm = volume_rays(orc, "head_scene")
    gpu_ctx.upload(named_case(orc, "head_scene")["flat"])
    n = len(o)
    dev = torch.device("cuda:0")
    t_o, t_d, t_tm = torch.from_numpy(o.copy()).to(dev), torch.from_numpy(d.copy()).to(dev), torch.from_numpy(tm).to(dev)
    for per_ray in (True, False):
        host = gpu_ctx.occluded_rays(o, d, t_max=7.0, ray_t_max=tm if per_ray else None, seed=SEED, first_key=11)
        t_out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        gpu_ctx.occluded_rays_device(n, t_o.data_ptr(), t_d.data_ptr(), t_out.data_ptr(), t_tm.data_ptr() if per_ray else None,
                                     t_max=7.0, seed=SEED, first_key=11)
        ms = gpu_ctx.last_kernel_ms()               # synchronises on the stop event
        torch.cuda.synchronize()
        out = t_out.cpu().numpy()
        assert ms > 0.0
        assert set(np.unique(out)) <= {0, 1}                                    # every byte written, 0 or 1
        assert np.array_equal(out != 0, host)
        assert host.any() and not host.all()


def test_a_ray_t_max_filled_with_the_scalar_equals_null(gpu_ctx, orc):
    sc = NAMED["config2"]()
    gpu_ctx.upload(sc.flatten())
    o, d = some_rays(orc, sc, 3000)
    for t_max in (INF, 4.0):
        plain = gpu_ctx.occluded_rays(o, d, t_max=t_max, seed=SEED, first_key=5)
        filled = gpu_ctx.occluded_rays(o, d, t_max=t_max, ray_t_max=np.full(len(o), t_max, F), seed=SEED, first_key=5)
        assert np.array_equal(plain, filled)
        assert plain.any() and not plain.all()


def test_host_form_chunks_a_large_batch(gpu_ctx, orc):
    """2^18 + 5 rays: two chunks of the host-pointer form, first_key and the ray_t_max slice advanced per chunk, against ONE device call."""
    import torch
    sc = NAMED["config1"]()
    gpu_ctx.upload(sc.flatten())
    o, d = some_rays(orc, sc, 4096)
    n = (1 << 18) + 5
    reps = n // 4096 + 1
    bo, bd = np.tile(o, (reps, 1))[:n].copy(), np.tile(d, (reps, 1))[:n].copy()
    tm = np.random.default_rng(5).choice(np.array([0.5, 2.0, 8.0, INF], F), n).astype(F)
    host = gpu_ctx.occluded_rays(bo, bd, ray_t_max=tm, seed=SEED, first_key=1)
    assert gpu_ctx.last_kernel_ms() > 0.0
    dev = torch.device("cuda:0")
    t_o, t_d, t_tm = torch.from_numpy(bo).to(dev), torch.from_numpy(bd).to(dev), torch.from_numpy(tm).to(dev)
    t_out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    gpu_ctx.occluded_rays_device(n, t_o.data_ptr(), t_d.data_ptr(), t_out.data_ptr(), t_tm.data_ptr(), seed=SEED, first_key=1)
    torch.cuda.synchronize()
    out = t_out.cpu().numpy()
    assert set(np.unique(out)) <= {0, 1}
    assert np.array_equal(out != 0, host)
    assert host[1 << 18:].shape == (5,) and host.any() and not host.all()


def test_refusals_and_trivial_cases(gpu_ctx, orc):
    lib = abi.load()
    sc = NAMED["config1"]()
    gpu_ctx.upload(sc.flatten())
    o, d = some_rays(orc, sc, 64)
    out = np.zeros(64, np.uint8)
    tm = np.full(64, 3.0, F)
    nan_tm = tm.copy()
    nan_tm[63] = np.nan
    h, po, pd, pout = gpu_ctx._h, o.ctypes.data, d.ctypes.data, out.ctypes.data
    nan = float("nan")

    def host(ctx=h, n=64, orig=po, dirs=pd, t_min=0.001, t_max=INF, rtm=None, res=pout):
        return lib.mi_occluded_rays(ctx, n, orig, dirs, t_min, t_max, rtm, SEED, 0, res)

    def device(ctx=h, n=64, orig=po, dirs=pd, t_min=0.001, t_max=INF, rtm=None, res=pout):
        return lib.mi_occluded_rays_device(ctx, n, orig, dirs, t_min, t_max, rtm, SEED, 0, res, None)

    assert host() == abi.MI_OK
    assert host(rtm=tm.ctypes.data) == abi.MI_OK
    assert host(rtm=np.full(64, INF, F).ctypes.data) == abi.MI_OK              # +inf is legal
    for call in (host, device):                                                # what both forms check (nothing is launched on a refusal)
        assert call(t_min=nan) == abi.MI_ERR_INVALID
        assert call(t_max=nan) == abi.MI_ERR_INVALID
        assert call(ctx=None) == abi.MI_ERR_INVALID
        assert call(orig=None) == abi.MI_ERR_INVALID
        assert call(dirs=None) == abi.MI_ERR_INVALID
        assert call(res=None) == abi.MI_ERR_INVALID
    assert host(rtm=nan_tm.ctypes.data) == abi.MI_ERR_INVALID                  # the host form reads ray_t_max
    # n_rays == 0: MI_OK, nothing launched, nothing written
    out[:] = 9
    assert host(n=0) == abi.MI_OK and device(n=0) == abi.MI_OK and np.all(out == 9)
    empty = gpu_ctx.occluded_rays(np.zeros((0, 3)), np.zeros((0, 3)), ray_t_max=np.zeros(0, F))
    assert empty.shape == (0,) and empty.dtype == bool
    with pytest.raises(ValueError):
        gpu_ctx.occluded_rays(o, d, ray_t_max=nan_tm)
    with pytest.raises(ValueError):
        gpu_ctx.occluded_rays(o, d, ray_t_max=tm[:63])
    # no scene uploaded
    fresh = Context(0)
    try:
        with pytest.raises(abi.MiError) as ei:
            fresh.occluded_rays(o, d)
        assert ei.value.code == abi.MI_ERR_NO_SCENE
        assert lib.mi_occluded_rays_device(fresh._h, 64, po, pd, 0.001, INF, None, SEED, 0, pout, None) == abi.MI_ERR_NO_SCENE
    finally:
        fresh.close()


def test_render_is_bit_identical_before_and_after_an_occlusion_query(gpu_ctx, orc):
    sc = scenes.config2(240, 136, 16, 10)
    gpu_ctx.upload(sc.flatten())
    a32, a8, asig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    o, d = some_rays(orc, sc, 5000)
    occ = gpu_ctx.occluded_rays(o, d, seed=SEED)
    occ2 = gpu_ctx.occluded_rays(o, d, ray_t_max=np.full(len(o), 2.0, F), seed=SEED)
    assert occ.any() and not occ2.all()
    b32, b8, bsig, _ = gpu_ctx.render(sc.camera, seed=1, want_sig=True)
    assert np.array_equal(a32.view(np.uint32), b32.view(np.uint32)) and np.array_equal(asig, bsig) and np.array_equal(a8, b8)
