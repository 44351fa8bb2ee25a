"""The float32 numpy statement of the multiband render calls (include/vmorph.h): what the kernels of
videomorphing_amd/csrc/vm_multiband.hip compute.  The two warped plates c0, c1 -- exactly what the render calls' tails form
before they blend: chain_ref.plates of the canvases' RGB or of the layers at the chain's two sampling positions -- and the
colour weight A (color_fa everywhere, or the plane k of transit_ref.transition_maps) are split into L + 1 frequency bands
by the 5-tap binomial reduce and expand of Burt and Adelson (1983); band l is blended under the weight plane of level l,
sharpened about 0.5 by sharp[l] >= 1, and the bands are summed from the coarsest up.  Every scalar is a float32, every
expression stands in the order written (the unit is built without contraction), fmaxf / fminf are np.fmax / np.fmin (a NaN
loses).  tests/test_multiband_ref.py pins the statement without a GPU; tests/test_gpu_multiband.py holds the kernels to it
bit for bit, level by level."""
import numpy as np

import chain_ref as C
import transit_ref
import warp_ref

f32 = np.float32
HALF, ONE, ZERO = f32(0.5), f32(1), f32(0)
MAX_LEVELS = 8
G0, G1, MASK, OUT = 0, 1, 2, 3          # vm_dbg_multiband_level's `what`
# (w, h, L), the smallest shapes at which the kernels can still go wrong: a coarsest level of 3 x 2 (the double fold at
# n = 2); one column or row past a tile edge at every level (twice); odd and even sizes in turn (45 -> 23 -> 12 -> 6,
# 27 -> 14 -> 7 -> 4); several tiles in both directions; five levels, nothing a power of two
SHAPES = [(9, 5, 2), (33, 17, 2), (65, 33, 3), (45, 27, 3), (77, 41, 4), (150, 97, 5)]


def fold(i, n):
    """reflect without repeating the edge sample: -1 -> 1, n -> n - 2; n >= 2 (two folds suffice for offsets of +-2)"""
    assert n >= 2
    while ((i < 0) | (i >= n)).any():
        i = np.where(i < 0, -i, i)
        i = np.where(i >= n, 2 * (n - 1) - i, i)
    return i


def red1(x, axis):
    """n -> m = (n + 1) // 2 along `axis`, centred on the even samples 2 i"""
    n = x.shape[axis]
    c = 2 * np.arange((n + 1) // 2)

    def t(d):
        return np.take(x, fold(c + d, n), axis=axis)

    return (f32(0.0625) * (t(-2) + t(2)) + f32(0.25) * (t(-1) + t(1))) + f32(0.375) * t(0)


def reduce(x):
    """along x first, then along y"""
    return red1(red1(x, 1), 0)


def exp1(x, n, axis):
    """m -> n along `axis`: i = o // 2, the taps folded into the coarse size m"""
    m = x.shape[axis]
    o = np.arange(n)
    i = o // 2

    def t(d):
        return np.take(x, fold(i + d, m), axis=axis)

    even = f32(0.125) * (t(-1) + t(1)) + f32(0.75) * t(0)
    odd = f32(0.5) * (t(0) + t(1))
    shape = [1] * x.ndim
    shape[axis] = n
    return np.where((o % 2 == 0).reshape(shape), even, odd)


def expand(x, w, h):
    """along x first, then along y"""
    return exp1(exp1(x, w, 1), h, 0)


def gauss(x, L):
    """[x, reduce(x), reduce(reduce(x)), ...]: L + 1 entries"""
    out = [np.ascontiguousarray(x, dtype=f32)]
    for _ in range(L):
        out.append(reduce(out[-1]))
    return out


def level_sizes(w, h, L):
    """[(w_l, h_l)] for l = 0..L: w_(l+1) = (w_l + 1) // 2"""
    out = [(w, h)]
    for _ in range(L):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def stages(c0, c1, A, sharp):
    """{(what, l): array} of everything the call forms: the Gaussian levels of c0, c1 and A, and R at every level"""
    c0, c1, A = np.asarray(c0, dtype=f32), np.asarray(c1, dtype=f32), np.asarray(A, dtype=f32)
    assert c0.ndim == 3 and c0.shape == c1.shape and A.shape == c0.shape[:2]
    sharp = [f32(s) for s in sharp]
    L = len(sharp) - 1
    assert 1 <= L <= MAX_LEVELS
    out = {}
    with np.errstate(all="ignore"):
        P0, P1, M = gauss(c0, L), gauss(c1, L), gauss(A, L)
        R = None
        for l in range(L, -1, -1):
            h_l, w_l = M[l].shape
            m = np.fmin(np.fmax(HALF + (M[l] - HALF) * sharp[l], ZERO), ONE)[..., None]
            if l == L:
                b0, b1 = P0[l], P1[l]
            else:
                b0, b1 = P0[l] - expand(P0[l + 1], w_l, h_l), P1[l] - expand(P1[l + 1], w_l, h_l)
            B = b0 * (ONE - m) + b1 * m
            R = B if l == L else expand(R, w_l, h_l) + B
            assert R.dtype == f32 and m.dtype == f32
            out[G0, l], out[G1, l], out[MASK, l], out[OUT, l] = P0[l], P1[l], M[l], R
    return out


def multiband(c0, c1, A, sharp):
    """(h, w, C) float32: the bands of c0 and c1 blended under the weight A"""
    return stages(c0, c1, A, sharp)[OUT, 0]


# ---- the plates: what the render calls' tails compute before they blend
def canvas_plates(ext0, ext1, ex, map0, map1):
    """chain_ref.tap of the extended canvases' RGB at (map + ex) + 0.5: two (h, w, 3) float32"""
    return C.plates(ext0[..., :3], ext1[..., :3], [(map0, map1)], ex)[0]


def layer_plates(layer0, layer1, map0, map1, lex=0):
    """the layers -- tight (lex = 0) or extended, the image at (lex, lex) -- sampled as warp_ref.render_layers samples
    them: two (h, w, C) float32"""
    return C.plates(layer0, layer1, [(map0, map1)], lex)[0]


def uniform_inputs(v, u, color_fa, geo_fa):
    """(map0, map1, A) of a uniform call"""
    map0, map1 = warp_ref.sampling_maps(v, u, geo_fa)[:2]
    return map0, map1, np.full(map0.shape[:2], f32(color_fa), f32)


def scheduled_inputs(v, u, sched_geo, sched_color, t, ease):
    """(map0, map1, A) of a call under a schedule: A is the plane k of transition_maps"""
    map0, map1, _, _, rates = transit_ref.transition_maps(v, u, sched_geo, sched_color, t, ease)
    return map0, map1, np.ascontiguousarray(rates[..., 1])


def render_bytes(ext0, ext1, ex, maps, sharp):
    """the RGB8 call on maps = (map0, map1, A) -> (h, w, 3) uint8: (uint8)((double)fminf(fmaxf(R, 0), 255) + 0.5),
    truncated; a NaN becomes 0"""
    c0, c1 = canvas_plates(ext0, ext1, ex, maps[0], maps[1])
    return C.bytes_of(multiband(c0, c1, maps[2], sharp), True)


def render_layers(layer0, layer1, maps, sharp, lex=0):
    """the layer call on maps = (map0, map1, A): float32 of the layers' shape (the extended layers': of the image's)"""
    c0, c1 = layer_plates(layer0, layer1, maps[0], maps[1], lex)
    return C.like(multiband(c0, c1, maps[2], sharp), layer0)
