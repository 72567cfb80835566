"""Hand-built images and guide tables for lightmap_finish / mi_lightmap_finish, shared by the host tests (which check what the helper
must do with them and that they notice mutants of it) and the GPU tests (which ask the kernels for the helper's bits on every one).

A battery is (name, image, points, normals, params): three [H, W, 3] float32 arrays and the keyword arguments of lightmap_finish.
Everything is built on the host from numpy and the host helper lightmap_texels; nothing here is ever fed anything the GPU made.  The
arrays are cached and read-only.

Colours are BASE = (1, 0.5, 2) times a power of two wherever a test asks for unchanged bits: a power of two scales through every rounding
of the weighted mean (sum(w c) == c sum(w) exactly), so a texel whose accepted taps all carry its own colour keeps its bits, and any
leak from a texel of another colour shows as a changed bit."""
import gzip
import inspect
import os

import numpy as np

from cs397raytracingsp22_amd import lightmap_texels, objload, tracing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
BASE = np.float32([1.0, 0.5, 2.0])
FACE_K = np.float32([0.25, 0.5, 1.0, 2.0, 4.0, 8.0])       # +x, -x, +y, -y, +z, -z
CUBE_SIZES = [(75, 41), (33, 65)]                          # both ragged against the 32-texel tile
_cache = {}


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def cube_mesh():
    if "mesh" not in _cache:
        with gzip.open(os.path.join(ROOT, "tests", "golden", "obj", "cube.obj.gz"), "rt") as fh:
            _cache["mesh"] = objload.load_obj_text(fh.read())[0]
    return _cache["mesh"]


def cube_table(W, H):
    """(points, normals, covered) of the cube's atlas at W x H: the centre table, from the host helper"""
    key = ("table", W, H)
    if key not in _cache:
        m = cube_mesh()
        _cache[key] = _frozen(*lightmap_texels(m.positions, m.normals, m.texcoords, m.indices, W, H))
    return _cache[key]


def cube_paint(W, H):
    """Every face a constant FACE_K[face] * BASE, the face chosen by the texel's normal; empty texels zero"""
    key = ("paint", W, H)
    if key not in _cache:
        _, N, covered = cube_table(W, H)
        axis = np.abs(N).argmax(axis=-1)
        negative = np.take_along_axis(N, axis[..., None], axis=-1)[..., 0] < 0
        img = (FACE_K[2 * axis + negative][..., None] * BASE).astype(np.float32)
        img[~covered] = 0.0
        _cache[key] = _frozen(img)[0]
    return _cache[key]


def cube_noisy(W, H):
    """cube_paint times 1 + 0.5 N(0, 1) per value, default_rng(1)"""
    key = ("noisy", W, H)
    if key not in _cache:
        noise = np.random.default_rng(1).standard_normal((H, W, 3))
        _cache[key] = _frozen((cube_paint(W, H) * (1.0 + 0.5 * noise)).astype(np.float32))[0]
    return _cache[key]


def flat_table(W, H, spacing=1.0):
    """A plane z = 0 facing +z, texel (x, y) at (x, y, 0) * spacing, every texel covered (writable copies)"""
    P = np.zeros((H, W, 3), np.float32)
    P[..., 0] = np.arange(W, dtype=np.float32)[None, :] * np.float32(spacing)
    P[..., 1] = np.arange(H, dtype=np.float32)[:, None] * np.float32(spacing)
    N = np.zeros((H, W, 3), np.float32)
    N[..., 2] = 1.0
    return P, N


def two_halves(W=40, H=8, gap=(0.0, 0.0, 0.0), k_left=1.0, k_right=4.0):
    """A flat table whose right half is moved by `gap`, the halves painted k_left * BASE and k_right * BASE"""
    P, N = flat_table(W, H)
    P[:, W // 2:] += np.float32(gap)
    img = np.empty((H, W, 3), np.float32)
    img[:, :W // 2] = np.float32(k_left) * BASE
    img[:, W // 2:] = np.float32(k_right) * BASE
    return _frozen(img, P, N)


def reach_battery(reach):
    """(c) coplanar halves with equal normals, 100 world units apart; one texel step spans 1"""
    img, P, N = two_halves(gap=(100.0, 0.0, 0.0))
    return (f"reach-{reach}", img, P, N, dict(levels=3, normal_power_log2=5, reach=reach, dilate=0))


def reach_equal_battery():
    """A noisy flat table with `reach` exactly one texel step: every tap's squared distance EQUALS its bound (small integers, exact in
    f32), so `<=` accepts all of them and `<` none but the centre"""
    P, N = flat_table(21, 13)
    img = (BASE * (1.0 + 0.25 * np.random.default_rng(2).standard_normal((13, 21, 3)))).astype(np.float32)
    return ("reach-equal", *_frozen(img, P, N), dict(levels=2, normal_power_log2=1, reach=1.0, dilate=0))


def plane_battery(sigma_plane):
    """(d) parallel halves, the right one lifted by 1 along the normal"""
    img, P, N = two_halves(gap=(0.0, 0.0, 1.0))
    return (f"plane-{sigma_plane}", img, P, N, dict(levels=3, normal_power_log2=5, sigma_plane=sigma_plane, dilate=0))


def colour_battery(sigma_color):
    """(e) one plane, a step edge in colour only"""
    img, P, N = two_halves()
    return (f"colour-{sigma_color}", img, P, N, dict(levels=3, normal_power_log2=5, sigma_color=sigma_color, dilate=0))


def colour_noisy_battery():
    """The noisy cube with a finite colour sigma over three levels: the sigma's division by the step shows in the bits"""
    W, H = CUBE_SIZES[1]
    P, N, _ = cube_table(W, H)
    return ("colour-noisy", cube_noisy(W, H), P, N, dict(levels=3, normal_power_log2=5, sigma_color=6.0, dilate=0))


def single_texel_battery(dilate=3):
    """(f) one covered texel in the middle of 9 x 9"""
    P, N = flat_table(9, 9)
    N[...] = 0.0
    N[4, 4] = (0.0, 0.0, 1.0)
    img = np.zeros((9, 9, 3), np.float32)
    img[4, 4] = np.float32(2.0) * BASE
    return (f"single-texel-{dilate}", *_frozen(img, P, N), dict(levels=0, dilate=dilate))


ISLANDS = ((2, 2, 1.0), (2, 6, 4.0))           # (y, x, k) in a 5 x 9 image: they meet in column 4


def islands_battery(dilate=3):
    """(f) two one-texel islands of different colour, Chebyshev distance 4 apart"""
    P, N = flat_table(9, 5)
    N[...] = 0.0
    img = np.zeros((5, 9, 3), np.float32)
    for y, x, k in ISLANDS:
        N[y, x] = (0.0, 0.0, 1.0)
        img[y, x] = np.float32(k) * BASE
    return (f"islands-{dilate}", *_frozen(img, P, N), dict(levels=0, dilate=dilate))


def limiting_batteries():
    """(g) a masked copy (empty texels of the input hold rubbish), 1 x 1, an all-empty table"""
    W, H = CUBE_SIZES[0]
    P, N, covered = cube_table(W, H)
    rubbish = cube_noisy(W, H).copy()
    rubbish[~covered] = 7.0
    one = (np.float32(0.5) * BASE).reshape(1, 1, 3)                  # a power of two times BASE: (w c) / w == c exactly
    P1, N1 = flat_table(1, 1)
    Pe, Ne = flat_table(37, 5)
    Ne[...] = 0.0
    Ne[1, 3] = (-0.0, 0.0, -0.0)                                      # either sign of zero is empty
    img_e = np.full((5, 37, 3), 3.0, np.float32)
    return [("masked-copy", *_frozen(rubbish), P, N, dict(levels=0, dilate=0)),
            ("one-by-one", *_frozen(one, P1, N1), dict(levels=3, dilate=4)),
            ("all-empty", *_frozen(img_e, Pe, Ne), dict(levels=3, dilate=4))]


def cube_batteries(levels=3, dilate=0):
    out = []
    for W, H in CUBE_SIZES:
        P, N, _ = cube_table(W, H)
        out.append((f"cube-flat-{W}x{H}-l{levels}-d{dilate}", cube_paint(W, H), P, N, dict(levels=levels, normal_power_log2=5, dilate=dilate)))
        out.append((f"cube-noisy-{W}x{H}-l{levels}-d{dilate}", cube_noisy(W, H), P, N, dict(levels=levels, normal_power_log2=5, dilate=dilate)))
    return out


def ragged_battery(W, H, levels=4, dilate=2):
    """A wavy, noisy surface with a quarter of its texels empty and every weight in play (finite sigmas and reach): for tile edges"""
    key = ("ragged", W, H)
    if key not in _cache:
        rng = np.random.default_rng(1000 * W + H)
        P, N = flat_table(W, H, 0.5)
        P[..., 2] = (0.3 * np.sin(0.4 * P[..., 0]) * np.cos(0.3 * P[..., 1])).astype(np.float32)
        N += (0.2 * rng.standard_normal((H, W, 3))).astype(np.float32)
        N /= np.sqrt((N * N).sum(axis=-1, keepdims=True)).astype(np.float32)
        empty = rng.random((H, W)) < 0.25
        N[empty] = 0.0
        P[empty] = 0.0
        img = (BASE * (1.0 + 0.3 * rng.standard_normal((H, W, 3)))).astype(np.float32)
        img[empty] = 0.0
        _cache[key] = _frozen(img, P, N)
    return (f"ragged-{W}x{H}-l{levels}-d{dilate}", *_cache[key],
            dict(levels=levels, normal_power_log2=2, sigma_plane=0.5, reach=1.5, sigma_color=4.0, dilate=dilate))


def all_batteries(cube_levels=3, cube_dilate=0):
    """Every battery, each (name, image, points, normals, params)"""
    return (cube_batteries(cube_levels, cube_dilate) +
            [reach_battery(INF), reach_battery(2.0), reach_equal_battery(), plane_battery(0.05), plane_battery(INF),
             colour_battery(0.5), colour_battery(INF), colour_noisy_battery(), single_texel_battery(), islands_battery()] +
            limiting_batteries())


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- mutants of the definitions
def mutant(helper, blocks, old, new):
    """`helper` (a public definition of tracing.py) made again from its own source and that of `blocks`, the building blocks it is
    composed of, with the text `old`, which must occur exactly once in all of it, replaced by `new`.  Everything is executed in one scope,
    so the copy calls the copies of its blocks: a mutant of a shared block is a mutant of every helper built on it."""
    src = "\n\n".join(inspect.getsource(f) for f in tuple(blocks) + (helper,))
    assert src.count(old) == 1, old
    scope = dict(vars(tracing))
    exec(compile(src.replace(old, new), f"<mutant of {helper.__name__}>", "exec"), scope)
    return scope[helper.__name__]


# the blocks of lightmap_finish and lightmap_finish_sh, of lightmap_finish_var, of lightmap_select
FINISH_BLOCKS = (tracing._lm_covered, tracing._lmf_level, tracing._lmf_dilate, tracing._check_finish_passes, tracing._lmf_finish)
VAR_BLOCKS = (tracing._lm_covered, tracing._lmv_variance, tracing._lmv_blur, tracing._lmf_level, tracing._lmf_dilate, tracing._check_finish_passes)
SELECT_BLOCKS = (tracing._lm_covered, tracing._lmv_variance, tracing._lmv_blur)

# one-token mutants of the blocks that lightmap_finish, lightmap_finish_sh and lightmap_finish_var share: each form's batteries notice each
LEVEL_AND_DILATION_MUTANTS = {
    "tap order reversed": ("for dy, dx in _LMF_TAPS:", "for dy, dx in _LMF_TAPS[::-1]:"),
    "H5's 3/8 and 1/4 swapped": ("f32(0.25), f32(0.375), f32(0.25)", "f32(0.375), f32(0.25), f32(0.375)"),
    "reach test exclusive": ("(d2 <= rr", "(d2 < rr"),
    "plane distance without fabsf": ("dpl = np.abs(", "dpl = ("),
    "dilation reads the in-pass state": ("valid.copy(), cur.copy()", "valid, cur"),
}
# of the two that lightmap_finish_var (constant and per-texel counts) and lightmap_select share
VARIANCE_MUTANTS = {
    "n for n - 1": ("d = np.maximum(n - 1, 1).astype(f32)", "d = np.maximum(n, 1).astype(f32)"),
    "blur includes empty neighbours": ("btake = covered & _lm_covered(nq)", "btake = covered"),
}
