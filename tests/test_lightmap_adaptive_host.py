"""The adaptive lightmap bake on the host: what the numpy helpers lightmap_select, lightmap_gather and lightmap_merge (the definitions of
mi_lightmap_select / _gather / _merge) and lightmap_finish_var with a counts plane must do with the batteries of adaptive_batteries.py,
that those batteries notice one-token mutants of the helpers, and the refusals of the new entry points that need no device.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

from cs397raytracingsp22_amd import abi, lightmap_finish_var, lightmap_gather, lightmap_merge, lightmap_select, tracing

import adaptive_batteries as ab
import finish_batteries as fb
import variance_batteries as vb
from adaptive_batteries import INF, bits

_ref = {}


def select(battery, fn=lightmap_select, **kw):
    _, img, m2, cnt, _, N, trel, tabs = battery
    return fn(img, m2, cnt, N, trel, tabs, **kw)


def reference(battery):
    if battery[0] not in _ref:
        _ref[battery[0]] = select(battery)
    return _ref[battery[0]]


def covered_of(battery):
    return (battery[5] != 0).any(axis=-1)


# ---------------------------------------------------------------- the batteries themselves
@pytest.mark.parametrize("battery", ab.all_batteries(), ids=lambda b: b[0])
def test_every_battery_selects_some_texels_but_not_all(battery):
    index, count, err = reference(battery)
    covered = int(covered_of(battery).sum())
    print(f"{battery[0]}: {count} of {covered} covered texels selected")
    assert 0.05 * covered <= count <= 0.95 * covered


def test_the_block_batteries_straddle_the_compaction_block():
    assert [b[1].shape[0] * b[1].shape[1] for b in ab.block_batteries()] == [1023, 1024, 1025, 2049]
    assert [b[1].shape[:2] for b in ab.tile_batteries()] == [(33, 31), (33, 32), (33, 33), (33, 65)]
    kinds = {b[0].rsplit("-", 1)[1] for b in ab.all_batteries()}
    assert kinds == {"uniform", "mixed", "single"}
    mixed = ab.ragged_battery(33, 33, "mixed")[3]
    assert (mixed == 0).any() and (mixed == 1).any() and (mixed >= 2).any()


def test_the_extremes():
    none, every, flat = ab.extreme_batteries()
    index, count, err = select(none)
    assert count == 0 and index.size == 0 and np.isinf(err).any()           # even the texels without information stay
    index, count, err = select(every)
    covered = covered_of(every)
    assert count == int((covered & (err > 0)).sum()) == int(covered.sum())
    assert np.array_equal(index, np.flatnonzero(covered & (err > 0)))
    index, count, err = select(flat)
    assert count == 0 and not err.any()


# ---------------------------------------------------------------- select
@pytest.mark.parametrize("battery", ab.block_batteries() + ab.cube_batteries()[:3], ids=lambda b: b[0])
def test_select_properties(battery):
    _, img, m2, cnt, P, N, trel, tabs = battery
    index, count, err = reference(battery)
    covered = covered_of(battery)
    H, W = covered.shape
    assert index.dtype == np.uint32 and err.dtype == np.float32 and err.shape == (H, W)
    assert (np.diff(index.astype(np.int64)) > 0).all()                       # ascending, no duplicates
    mask = np.zeros(H * W, bool)
    mask[index] = True
    assert count == int(mask.sum()) == index.size
    assert not mask.reshape(H, W)[~covered].any() and not bits(err)[~covered].any()
    lum = (np.abs(img[..., 0]) + np.abs(img[..., 1])) + np.abs(img[..., 2])
    with np.errstate(all="ignore"):
        assert np.array_equal(mask.reshape(H, W), covered & (err > np.float32(trel) * lum + np.float32(tabs)))
    # a texel without information is always selected, and so are its covered neighbours (the blur carries the infinity)
    few = covered & (cnt < 2)
    assert mask.reshape(H, W)[few].all() and np.isinf(err[few]).all()
    # truncation keeps the lowest indices; the count does not change
    for cap in (0, 1, count - 1, count, count + 5):
        part, n, _ = select(battery, capacity=cap)
        assert n == count and np.array_equal(part, index[:cap])


def test_error_is_the_blurred_standard_error_of_the_texels_own_count():
    """A flat table with uniform counts, constant mean 1 and m2 = 1.25: v_c = 0.25 / (n - 1) per channel and the blur of a constant is
    that constant, with every weight a power of two: sd = sqrt(0.75 / (n - 1)) exactly"""
    _, img, m2, _, P, N, _ = vb.propagation_battery()
    for n in (2, 4, 5):
        cnt = np.full(img.shape[:2], n, np.uint32)
        _, _, err = lightmap_select(img, m2, cnt, N, 0.0, 0.0)
        want = np.sqrt(np.float32(0.75) / np.float32(n - 1))
        assert np.array_equal(bits(err), bits(np.full(err.shape, want, np.float32)))


def test_a_non_finite_texel_changes_selection_within_distance_one():
    b = ab.cube_batteries()[3]                          # 75 x 41, noisy, uniform counts
    _, clean, m2, cnt, P, N, trel, tabs = b
    covered = covered_of(b)
    H, W = covered.shape
    ys, xs = np.nonzero(covered)
    k = int(np.argmin(np.maximum(np.abs(ys - H // 2), np.abs(xs - W // 2))))
    y0, x0 = int(ys[k]), int(xs[k])
    yy, xx = np.mgrid[0:H, 0:W]
    far = (np.maximum(np.abs(yy - y0), np.abs(xx - x0)) > 1).reshape(-1)
    want = np.zeros(H * W, bool)
    want[reference(b)[0]] = True
    for which, value in ((0, np.nan), (1, np.inf), (0, -np.inf), (1, np.nan)):
        dirty = [clean.copy(), m2.copy()]
        dirty[which][y0, x0] = value
        index, _, err = lightmap_select(dirty[0], dirty[1], cnt, N, trel, tabs)
        got = np.zeros(H * W, bool)
        got[index] = True
        assert np.array_equal(got[far], want[far])
        assert np.array_equal(bits(err).reshape(-1)[far], bits(reference(b)[2]).reshape(-1)[far])


# ---------------------------------------------------------------- gather and merge
@pytest.mark.parametrize("cw", [1, 7, 1024])
def test_gather_round_trips(cw):
    b = ab.ragged_battery(65, 33)
    _, img, m2, cnt, P, N, _, _ = b
    index = reference(b)[0]
    rows = 3
    Pr = np.stack([P + np.float32(r) for r in range(rows)])
    Nr = np.stack([N * np.float32(r + 1) for r in range(rows)])
    cp, cn = lightmap_gather(index, Pr, Nr, cw)
    n, ch = index.size, (index.size + cw - 1) // cw
    assert cp.shape == cn.shape == (rows, ch, cw, 3) and cp.dtype == np.float32
    flat_p, flat_n = cp.reshape(rows, -1, 3), cn.reshape(rows, -1, 3)
    assert np.array_equal(bits(flat_p[:, :n]), bits(Pr.reshape(rows, -1, 3)[:, index]))
    assert np.array_equal(bits(flat_n[:, :n]), bits(Nr.reshape(rows, -1, 3)[:, index]))
    assert not bits(flat_p[:, n:]).any() and not bits(flat_n[:, n:]).any()          # the empty-texel mark behind the list
    # a "render" that returns the gathered points, merged into planes of zeros with zero counts, puts every point back where it came from
    H, W = img.shape[:2]
    zeros = np.zeros((H, W, 3), np.float32)
    back, back_n, c2 = lightmap_merge(index, cp[0], cn[0], 4, zeros, zeros, np.zeros((H, W), np.uint32))
    sel = np.zeros(H * W, bool)
    sel[index] = True
    assert np.array_equal(bits(back.reshape(-1, 3)[sel]), bits((P + np.float32(0)).reshape(-1, 3)[sel])) and not bits(back.reshape(-1, 3)[~sel]).any()
    assert np.array_equal(bits(back_n.reshape(-1, 3)[sel]), bits(N.reshape(-1, 3)[sel]))
    assert np.array_equal(c2.reshape(-1), np.where(sel, 4, 0))
    # a three-dimensional table is one row
    one_p, one_n = lightmap_gather(index, P, N, cw)
    assert np.array_equal(bits(one_p), bits(lightmap_gather(index, P[None], N[None], cw)[0])) and one_n.shape == (1, ch, cw, 3)


def test_gather_wild_index_gives_an_empty_slot():
    _, img, m2, cnt, P, N, _, _ = ab.ragged_battery(31, 33)
    H, W = img.shape[:2]
    live = int(np.flatnonzero((N != 0).any(axis=-1).reshape(-1))[5])
    index = np.uint32([live, W * H, 0xffffffff, live + 1])
    cp, cn = lightmap_gather(index, P, N, 7)
    assert cp.shape == (1, 1, 7, 3) and cn[0, 0, 0].any()
    assert not bits(cp[0, 0, 1:3]).any() and not bits(cn[0, 0, 1:3]).any() and not bits(cp[0, 0, 4:]).any()
    assert np.array_equal(bits(cp[0, 0, 3]), bits(P.reshape(-1, 3)[live + 1]))


@pytest.mark.parametrize("battery", [ab.ragged_battery(65, 33), ab.cube_batteries()[4]], ids=lambda b: b[0])
def test_merge_properties(battery):
    _, img, m2, cnt, P, N, _, _ = battery
    index = reference(battery)[0]
    H, W = img.shape[:2]
    S = 4
    mean, m2r = ab.round_for(battery, index, S)
    out, out_m2, out_cnt = lightmap_merge(index, mean, m2r, S, img, m2, cnt)
    sel = np.zeros(H * W, bool)
    sel[index] = True
    flat = lambda a: a.reshape(H * W, -1)                                                     # noqa: E731
    assert np.array_equal(bits(flat(out)[~sel]), bits(flat(img)[~sel])) and np.array_equal(bits(flat(out_m2)[~sel]), bits(flat(m2)[~sel]))
    assert np.array_equal(out_cnt.reshape(-1), cnt.reshape(-1) + np.where(sel, S, 0)) and out_cnt.dtype == np.uint32
    # the merged value, one texel at a time in plain f32 scalars
    f32 = np.float32
    for i in (0, index.size // 2, index.size - 1):
        t = int(index[i])
        n0 = f32(int(cnt.reshape(-1)[t]))
        for plane, new, got in ((img, mean, out), (m2, m2r, out_m2)):
            for k in range(3):
                want = (n0 * plane.reshape(-1, 3)[t, k] + f32(S) * new[i, k]) / f32(int(cnt.reshape(-1)[t]) + S)
                assert bits(np.float32(want)) == bits(got.reshape(-1, 3)[t, k])
    assert (bits(flat(out)[sel]) != bits(flat(img)[sel])).any()
    # the inputs are not written
    assert not img.flags.writeable and not cnt.flags.writeable
    # a wild index is skipped
    wild = np.concatenate([index[:3], np.uint32([W * H, 0xffffffff])])
    a = lightmap_merge(wild, mean[:5], m2r[:5], S, img, m2, cnt)
    b = lightmap_merge(index[:3], mean[:3], m2r[:3], S, img, m2, cnt)
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    # an empty list changes nothing
    c = lightmap_merge(np.zeros(0, np.uint32), mean[:0], m2r[:0], S, img, m2, cnt)
    assert np.array_equal(bits(c[0]), bits(img)) and np.array_equal(c[2], cnt)


def test_merging_a_texels_own_estimate_changes_it_by_at_most_one_ulp():
    for battery in (ab.ragged_battery(65, 33), ab.cube_batteries()[4]):
        _, img, m2, cnt, P, N, _, _ = battery
        index = reference(battery)[0]
        index = index[cnt.reshape(-1)[index] > 0]                       # a texel without samples has no estimate of its own
        for S in (1, 3, 4, 7):
            out, out_m2, _ = lightmap_merge(index, img.reshape(-1, 3)[index], m2.reshape(-1, 3)[index], S, img, m2, cnt)
            for got, was in ((out, img), (out_m2, m2)):
                d = np.abs(bits(got).astype(np.int64) - bits(was).astype(np.int64))
                print(f"{battery[0]} S'={S}: largest change {int(d.max())} ulp")
                assert int(d.max()) <= 1


# ---------------------------------------------------------------- the finish with counts
def test_finish_with_a_constant_plane_is_the_scalar_finish():
    for b in vb.cube_batteries(3, 2)[:2] + [vb.ragged_battery(33, 33)]:
        _, img, m2, S, P, N, params = b
        want = lightmap_finish_var(img, m2, S, P, N, **params)
        for dtype in (np.uint32, np.int64):
            got = lightmap_finish_var(img, m2, np.full(img.shape[:2], S, dtype), P, N, **params)
            assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])


def test_finish_with_counts_uses_the_texels_own_count():
    b = ab.ragged_battery(33, 33, "mixed")
    _, img, m2, cnt, P, N, _, _ = b
    out, var, valid = lightmap_finish_var(img, m2, cnt, P, N, levels=0, dilate=0)
    covered = covered_of(b)
    f32 = np.float32
    for y, x in list(zip(*np.nonzero(covered)))[::37]:
        n = int(cnt[y, x])
        if n < 2:
            assert bits(var[y, x]) == 0
            continue
        v = [np.fmax(f32(0), m2[y, x, k] - img[y, x, k] * img[y, x, k]) / f32(n - 1) for k in range(3)]
        assert bits(f32((v[0] + v[1]) + v[2])) == bits(var[y, x])
    assert not bits(var)[~covered].any() and (var[covered & (cnt < 2)] == 0).all() and (var[covered & (cnt >= 2)] > 0).any()
    # two planes that differ in one texel's count give different variances there
    other = cnt.copy()
    y, x = [int(v[0]) for v in np.nonzero(covered & (cnt >= 2))]
    other[y, x] += 3
    assert bits(lightmap_finish_var(img, m2, other, P, N, levels=0, dilate=0)[1][y, x]) != bits(var[y, x])


def test_finish_with_counts_notices_n_for_n_minus_one():
    """The initial variance is one block for the constant and the per-texel n: its mutant shows in the counts form on every battery
    whose variance is not zero (lightmap_select's batteries notice it below, the constant form's in test_lightmap_variance_host.py)"""
    wrong = fb.mutant(lightmap_finish_var, fb.VAR_BLOCKS, *fb.VARIANCE_MUTANTS["n for n - 1"])
    noticed = []
    for b in vb.all_batteries(3, 2):
        _, img, m2, S, P, N, params = b
        cnt = np.full(img.shape[:2], S, np.uint32)
        x, y = lightmap_finish_var(img, m2, cnt, P, N, **params), wrong(img, m2, cnt, P, N, **params)
        if not all(np.array_equal(bits(p), bits(q)) for p, q in zip(x[:2], y[:2])):
            noticed.append(b[0])
    print(f"noticed by {noticed}")
    assert len(noticed) >= 8


# ---------------------------------------------------------------- refusals of the helpers
def test_bad_arguments_are_refused():
    _, img, m2, cnt, P, N, trel, tabs = ab.ragged_battery(31, 33)
    nan = float("nan")
    index = reference(ab.ragged_battery(31, 33))[0]
    mean, m2r = ab.round_for(ab.ragged_battery(31, 33), index)
    bad_select = [lambda: lightmap_select(img, m2, cnt, N, nan, tabs), lambda: lightmap_select(img, m2, cnt, N, trel, nan),
                  lambda: lightmap_select(img, m2, cnt, N, -0.1, tabs), lambda: lightmap_select(img, m2, cnt, N, trel, -1.0),
                  lambda: lightmap_select(img, m2[:4], cnt, N, trel, tabs), lambda: lightmap_select(img, m2, cnt[:4], N, trel, tabs),
                  lambda: lightmap_select(img, m2, cnt.astype(np.float32), N, trel, tabs),
                  lambda: lightmap_select(img, m2, cnt.astype(np.int64) - 1, N, trel, tabs),
                  lambda: lightmap_select(img, m2, cnt, N[..., :2], trel, tabs), lambda: lightmap_select(img, m2, cnt, N, trel, tabs, capacity=-1)]
    bad_gather = [lambda: lightmap_gather(index, P, N, 0), lambda: lightmap_gather(index, P, N, 32769),
                  lambda: lightmap_gather(index[:0], P, N, 7), lambda: lightmap_gather(index, P.astype(np.float64), N, 7),
                  lambda: lightmap_gather(index, P, N[:4], 7), lambda: lightmap_gather(index.astype(np.float32), P, N, 7),
                  lambda: lightmap_gather(index[None], P, N, 7), lambda: lightmap_gather(np.tile(index, 200), P, N, 1)]
    bad_merge = [lambda: lightmap_merge(index, mean, m2r, 0, img, m2, cnt), lambda: lightmap_merge(index, mean, m2r, 65536, img, m2, cnt),
                 lambda: lightmap_merge(index, mean[:3], m2r, 4, img, m2, cnt), lambda: lightmap_merge(index, mean, m2r[:3], 4, img, m2, cnt),
                 lambda: lightmap_merge(np.concatenate([index, index[:1]]), np.zeros((index.size + 1, 3), np.float32),
                                        np.zeros((index.size + 1, 3), np.float32), 4, img, m2, cnt),
                 lambda: lightmap_merge(index, mean, m2r, 4, img, m2[:4], cnt), lambda: lightmap_merge(index, mean, m2r, 4, img, m2, cnt[:, :4])]
    bad_finish = [lambda: lightmap_finish_var(img, m2, cnt[:4], P, N), lambda: lightmap_finish_var(img, m2, cnt.astype(np.float32), P, N)]
    for k, call in enumerate(bad_select + bad_gather + bad_merge + bad_finish):
        with pytest.raises(ValueError):
            call()
            print("not refused:", k)
    # the limits themselves are legal
    lightmap_select(img, m2, cnt, N, 0.0, INF, capacity=0)
    lightmap_select(img, m2, cnt, N, INF, 0.0)
    lightmap_gather(index, P, N, 32768)
    lightmap_merge(index, mean, m2r, 65535, img, m2, cnt)


# ---------------------------------------------------------------- mutants
SELECT_MUTANTS = {
    **fb.VARIANCE_MUTANTS,
    ">= for >": ("selected = covered & (sd > thr)", "selected = covered & (sd >= thr)"),
    "no blur": ("sd = np.where(covered, np.sqrt(bs / bw), zero)", "sd = np.where(covered, np.sqrt(V), zero)"),
    "a texel without samples counts as converged": ("_lmv_variance(img, M2, cnt, covered, f32(np.inf))", "_lmv_variance(img, M2, cnt, covered, f32(0.0))"),
}
MERGE_MUTANTS = {
    "weights swapped": ("plane[t] = (n0 * a + Sf * b) / tot", "plane[t] = (Sf * a + n0 * b) / tot"),
    "divided by the old count": ("tot = n0_int.astype(f32)[:, None], f32(S), (n0_int + S).astype(f32)[:, None]",
                                 "tot = n0_int.astype(f32)[:, None], f32(S), (n0_int + 0).astype(f32)[:, None]"),
}


def mutant(fn, old, new):
    return fb.mutant(fn, fb.SELECT_BLOCKS if fn is lightmap_select else (), old, new)


def same_selection(x, y):
    return np.array_equal(x[0], y[0]) and x[1] == y[1] and np.array_equal(bits(x[2]), bits(y[2]))


def noticing_batteries():
    return ab.all_batteries() + ab.extreme_batteries()


def test_unmutated_copies_are_the_helpers():
    copy = mutant(lightmap_select, "thr = trel * lum + tabs", "thr = trel * lum + tabs")
    for b in noticing_batteries():
        assert same_selection(select(b, copy), reference(b) if b in ab.all_batteries() else select(b)), b[0]


@pytest.mark.parametrize("name", list(SELECT_MUTANTS))
def test_batteries_notice_select_mutants(name):
    """At least one battery's list, count or error plane differs between the helper and the mutant"""
    wrong = mutant(lightmap_select, *SELECT_MUTANTS[name])
    noticed = [b[0] for b in noticing_batteries() if not same_selection(select(b, wrong), select(b))]
    print(f"{name}: noticed by {len(noticed)} batteries, {noticed[:4]}")
    assert noticed


@pytest.mark.parametrize("name", list(MERGE_MUTANTS))
def test_batteries_notice_merge_mutants(name):
    wrong = mutant(lightmap_merge, *MERGE_MUTANTS[name])
    noticed = []
    for b in ab.block_batteries():
        _, img, m2, cnt, _, _, _, _ = b
        index = reference(b)[0]
        mean, m2r = ab.round_for(b, index)
        with np.errstate(all="ignore"):
            x, y = lightmap_merge(index, mean, m2r, 4, img, m2, cnt), wrong(index, mean, m2r, 4, img, m2, cnt)
        if not all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(x, y)):
            noticed.append(b[0])
    print(f"{name}: noticed by {noticed}")
    assert noticed


# ---------------------------------------------------------------- the library's refusals that need no device
def test_refusals_come_before_the_context():
    lib = abi.load()
    b = ab.ragged_battery(31, 33)
    _, img, m2, cnt, P, N, trel, tabs = b
    H, W = img.shape[:2]
    index_ref = reference(b)[0]
    n = index_ref.size
    mean, m2r = ab.round_for(b, index_ref)
    out_index = np.full(W * H, 0xABCDABCD, np.uint32)
    out_count = np.full(1, 0xABCDABCD, np.uint32)
    out_err = np.full((H, W), -7.0, np.float32)
    cp = np.full((1, (n + 6) // 7, 7, 3), -7.0, np.float32)
    cn = cp.copy()
    image, moments, counts = img.copy(), m2.copy(), cnt.copy()
    nan = float("nan")
    a = lambda x: None if x is None else x.ctypes.data                                          # noqa: E731

    def sel(device, w=W, h=H, image_=img, m2_=m2, counts_=cnt, normals=N, trel_=trel, tabs_=tabs, cap=W * H, index=out_index, count=out_count):
        args = (None, w, h, a(image_), a(m2_), a(counts_), a(normals), trel_, tabs_, cap, a(index), a(count), a(out_err))
        rc = lib.mi_lightmap_select_device(*args, None) if device else lib.mi_lightmap_select(*args)
        return rc, lib.mi_last_error().decode()

    def gat(device, w=W, h=H, rows=1, n_=n, index=index_ref, points=P, normals=N, cw=7, out_p=cp, out_n=cn):
        args = (None, w, h, rows, n_, a(index), a(points), a(normals), cw, a(out_p), a(out_n))
        rc = lib.mi_lightmap_gather_device(*args, None) if device else lib.mi_lightmap_gather(*args)
        return rc, lib.mi_last_error().decode()

    def mer(device, w=W, h=H, n_=n, index=index_ref, mean_=mean, m2r_=m2r, S=4, image_=image, m2_=moments, counts_=counts):
        args = (None, w, h, n_, a(index), a(mean_), a(m2r_), S, a(image_), a(m2_), a(counts_))
        rc = lib.mi_lightmap_merge_device(*args, None) if device else lib.mi_lightmap_merge(*args)
        return rc, lib.mi_last_error().decode()

    refused = [(sel, dict(image_=None), "required"), (sel, dict(m2_=None), "required"), (sel, dict(counts_=None), "required"),
               (sel, dict(normals=None), "required"), (sel, dict(count=None), "required"), (sel, dict(index=None), "out_index"),
               (sel, dict(w=0), "width"), (sel, dict(h=32769), "width"), (sel, dict(trel_=nan), "target_rel"), (sel, dict(trel_=-1.0), "target_rel"),
               (sel, dict(tabs_=nan), "target_abs"), (sel, dict(tabs_=-0.5), "target_abs"),
               (gat, dict(index=None), "required"), (gat, dict(points=None), "required"), (gat, dict(normals=None), "required"),
               (gat, dict(out_p=None), "required"), (gat, dict(out_n=None), "required"), (gat, dict(w=0), "width"), (gat, dict(h=0), "width"),
               (gat, dict(rows=0), "rows"), (gat, dict(rows=65536), "rows"), (gat, dict(cw=0), "cw"), (gat, dict(cw=32769), "cw"),
               (gat, dict(n_=0), "rows of slots"), (gat, dict(n_=32769, cw=1), "rows of slots"),
               (mer, dict(index=None), "required"), (mer, dict(mean_=None), "required"), (mer, dict(m2r_=None), "required"),
               (mer, dict(image_=None), "required"), (mer, dict(m2_=None), "required"), (mer, dict(counts_=None), "required"),
               (mer, dict(w=32769), "width"), (mer, dict(S=0), "round_samples"), (mer, dict(S=65536), "round_samples")]
    for device in (False, True):
        for fn, kw, word in refused:
            rc, msg = fn(device, **kw)
            assert rc == abi.MI_ERR_INVALID and word in msg and "ctx" not in msg, (fn.__name__, kw, device, msg)
        for fn, kw in ((sel, dict()), (sel, dict(cap=0, index=None, tabs_=INF)), (gat, dict()), (gat, dict(cw=32768)), (mer, dict()),
                       (mer, dict(S=65535)), (mer, dict(n_=0))):
            rc, msg = fn(device, **kw)
            assert rc == abi.MI_ERR_INVALID and msg == "ctx is NULL", (fn.__name__, kw, device, msg)
    # the host form of merge can see a texel listed twice
    twice = np.concatenate([index_ref, index_ref[2:3]])
    rc, msg = mer(False, n_=twice.size, index=twice, mean_=np.zeros((twice.size, 3), np.float32), m2r_=np.zeros((twice.size, 3), np.float32))
    assert rc == abi.MI_ERR_INVALID and "twice" in msg
    assert (out_index == 0xABCDABCD).all() and out_count[0] == 0xABCDABCD and (out_err == -7.0).all() and (cp == -7.0).all() and (cn == -7.0).all()
    assert np.array_equal(bits(image), bits(img)) and np.array_equal(bits(moments), bits(m2)) and np.array_equal(counts, cnt)


def test_finish_var_counts_refusals_come_before_the_context():
    lib = abi.load()
    _, img, m2, cnt, P, N, _, _ = ab.ragged_battery(31, 33)
    H, W = img.shape[:2]
    out = np.full((H, W, 3), -7.0, np.float32)
    var = np.full((H, W), -7.0, np.float32)
    valid = np.full((H, W), 9, np.uint8)
    nan = float("nan")

    def call(device, w=W, h=H, image=img.ctypes.data, m2_=m2.ctypes.data, counts=cnt.ctypes.data, points=P.ctypes.data, normals=N.ctypes.data,
             levels=3, npow=5, sigma_plane=INF, reach=INF, sigma_color=8.0, color_floor=1e-6, dilate=4, out_image=out.ctypes.data,
             out_var=var.ctypes.data):
        args = (None, w, h, image, m2_, counts, points, normals, levels, npow, sigma_plane, reach, sigma_color, color_floor, dilate,
                out_image, out_var, valid.ctypes.data)
        rc = lib.mi_lightmap_finish_var_counts_device(*args, None) if device else lib.mi_lightmap_finish_var_counts(*args)
        return rc, lib.mi_last_error().decode()

    refused = [(dict(image=None), "required"), (dict(m2_=None), "required"), (dict(counts=None), "counts"), (dict(points=None), "required"),
               (dict(normals=None), "required"), (dict(out_image=None), "required"), (dict(w=0), "width"), (dict(h=32769), "width"),
               (dict(levels=9), "levels"), (dict(npow=8), "normal_power_log2"), (dict(dilate=257), "dilate"),
               (dict(sigma_plane=nan), "sigma_plane"), (dict(reach=0.0), "reach"), (dict(sigma_color=INF), "sigma_color"),
               (dict(color_floor=0.0), "color_floor")]
    for device in (False, True):
        for kw, word in refused:
            rc, msg = call(device, **kw)
            assert rc == abi.MI_ERR_INVALID and word in msg and "ctx" not in msg, (kw, device, msg)
        rc, msg = call(device)
        assert rc == abi.MI_ERR_INVALID and msg == "ctx is NULL"
    for kw in (dict(out_image=img.ctypes.data + 12), dict(out_var=cnt.ctypes.data), dict(out_image=cnt.ctypes.data + 4 * W * H - 4)):
        rc, msg = call(True, **kw)
        assert rc == abi.MI_ERR_INVALID and "overlaps" in msg, (kw, msg)
    assert (out == -7.0).all() and (var == -7.0).all() and (valid == 9).all()


def test_adaptive_bake_refusals_without_a_device():
    """out_m2, out_counts and the adaptive parameters are checked first; everything else is mi_bake_lightmap_moments', which begins at the
    context"""
    lib = abi.load()
    cam = tracing.Camera(screen_width=4, screen_height=3, aa_sample_count=2, path_depth=2).to_pod()
    opts = abi.mi_render_opts(seed=1, rank=0, world=1, variant=abi.MI_VARIANT_DEFAULT, want_signature=0, flags=0, max_state_bytes=0)
    m2 = np.full((3, 4, 3), -7.0, np.float32)
    counts = np.full((3, 4), 77, np.uint32)
    st = abi.mi_stats()
    mesh = abi.mi_mesh()
    nan = float("nan")

    def call(first=4, per_round=4, rounds=2, trel=0.1, tabs=0.0, ad=True, out_counts=counts.ctypes.data, out_m2=m2.ctypes.data):
        pod = abi.mi_lightmap_adaptive(first_samples=first, round_samples=per_round, max_rounds=rounds, target_rel=trel, target_abs=tabs)
        rc = lib.mi_bake_lightmap_adaptive(None, C.byref(cam), C.byref(opts), C.byref(mesh), 0, 0.0, C.byref(pod) if ad else None, out_counts,
                                           out_m2, None, None, None, None, C.byref(st))
        return rc, lib.mi_last_error().decode()

    for kw, word in ((dict(out_m2=None), "required"), (dict(out_counts=None), "required"), (dict(ad=False), "adaptive"),
                     (dict(first=1), "first_samples"), (dict(first=0), "first_samples"), (dict(first=65536), "first_samples"),
                     (dict(per_round=0), "round_samples"), (dict(per_round=65536), "round_samples"),
                     (dict(first=65535, per_round=65535, rounds=256), "2^24"), (dict(rounds=0xffffffff), "2^24"),
                     (dict(trel=nan), "target"), (dict(trel=-1.0), "target"), (dict(tabs=nan), "target"), (dict(tabs=-1e-3), "target")):
        rc, msg = call(**kw)
        assert rc == abi.MI_ERR_INVALID and word in msg and "ctx" not in msg, (kw, msg)
    for kw in (dict(), dict(first=2, per_round=1, rounds=0), dict(first=65535, per_round=65535, rounds=255), dict(trel=INF, tabs=INF)):
        rc, msg = call(**kw)
        assert rc == abi.MI_ERR_INVALID and msg == "ctx is NULL", (kw, msg)
    assert (m2 == -7.0).all() and (counts == 77).all()
    assert C.sizeof(abi.mi_lightmap_adaptive) == 20


def test_mirrors_name_the_new_calls():
    import os
    root = fb.ROOT
    hpp = open(os.path.join(root, "cs397raytracingsp22_amd", "host", "tracing.hpp")).read()
    assert "bake_lightmap_adaptive(" in hpp and "finish_lightmap_var_counts(" in hpp
    rs = open(os.path.join(root, "rust", "src", "util", "tracing_flatten.rs")).read()
    assert "pub fn bake_lightmap_adaptive(" in rs and "pub fn finish_lightmap_var_counts(" in rs
    for name in ("lightmap_select", "lightmap_select_device", "lightmap_gather", "lightmap_gather_device", "lightmap_merge",
                 "lightmap_merge_device", "lightmap_finish_var_counts", "lightmap_finish_var_counts_device", "bake_lightmap_adaptive"):
        assert callable(getattr(tracing.Context, name)), name
    assert "adaptive" in inspect.signature(tracing.Scene.bake_lightmap).parameters
