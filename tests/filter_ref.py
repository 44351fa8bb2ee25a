"""The float32 numpy statement of what videomorphing_amd/csrc/vm_filter.hip computes: the viewport calls of
tests/viewport_ref.py with a cubic filter on the taps that read picture content -- a canvas, a layer.  The chain and the
sample points are viewport_ref's (this module takes the `maps` of viewport_ref.sample_maps); the blend, the sum in sample
order and the division by (float)N are the tail of tests/chain_ref.py, handed this module's tap; what differs is that tap
and, for RGB8, the clamp of the mean to [0, 255] before the rounding (chain_ref.bytes_of with clamp).  A cubic tap reads a
W x H image at (x, y), the coordinates chain_ref.tap takes, in float32, in this order:

    xb = x - 0.5f;  fi = floorf(xb);  a = xb - fi;  fi = fminf(fmaxf(fi, -2.0f), (float)W + 1.0f);  i = (int)fi
    columns  c_k = clamp(i + k, 0, W - 1),  k = -1, 0, 1, 2                 (rows r_m from y, b, H likewise)
    inner(d) = ((p3 * d + p2) * d) * d + p0            outer(d) = ((q3 * d + q2) * d + q1) * d + q0
    wx_-1 = outer(1.0f + a)   wx_0 = inner(a)   wx_1 = inner(1.0f - a)   wx_2 = outer(2.0f - a)     (wy from b likewise)
    row_m = ((wx_-1 * t(c_-1, r_m) + wx_0 * t(c_0, r_m)) + wx_1 * t(c_1, r_m)) + wx_2 * t(c_2, r_m)
    value = ((wy_-1 * row_-1 + wy_0 * row_0) + wy_1 * row_1) + wy_2 * row_2

Every scalar is a float32 and every expression stands in the kernels' order (they are built without contraction).
tests/test_filter_ref.py pins the statement without a GPU, tests/test_gpu_filtered.py holds the kernels to it bit for bit."""
import numpy as np

import chain_ref as C
from chain_ref import HALF, ONE, f32

BILINEAR, CATMULL_ROM, MITCHELL, BSPLINE = 0, 1, 2, 3
CUBIC = (CATMULL_ROM, MITCHELL, BSPLINE)
# (p3, p2, p0, q3, q2, q1, q0), each (float)(n / d) of doubles
COEFFS = {
    CATMULL_ROM: tuple(f32(n / d) for n, d in ((3.0, 2.0), (-5.0, 2.0), (1.0, 1.0), (-1.0, 2.0), (5.0, 2.0), (-4.0, 1.0), (2.0, 1.0))),
    MITCHELL: tuple(f32(n / d) for n, d in ((7.0, 6.0), (-2.0, 1.0), (8.0, 9.0), (-7.0, 18.0), (2.0, 1.0), (-10.0, 3.0), (16.0, 9.0))),
    BSPLINE: tuple(f32(n / d) for n, d in ((1.0, 2.0), (-1.0, 1.0), (2.0, 3.0), (-1.0, 6.0), (1.0, 1.0), (-2.0, 1.0), (4.0, 3.0))),
}
TWO = f32(2)


def weights(a, filt):
    """(w_-1, w_0, w_1, w_2) of the four texels of one axis at the fraction a (float32, any shape)"""
    p3, p2, p0, q3, q2, q1, q0 = COEFFS[filt]
    a = np.asarray(a, dtype=f32)

    def inner(d):
        return ((p3 * d + p2) * d) * d + p0

    def outer(d):
        return ((q3 * d + q2) * d + q1) * d + q0

    with np.errstate(all="ignore"):
        w = (outer(ONE + a), inner(a), inner(ONE - a), outer(TWO - a))
    assert all(t.dtype == f32 for t in w)
    return w


def _axis(n, x):
    """the fraction and the four clamped texel indices of one axis of n texels"""
    xb = x - HALF
    fi = np.floor(xb)
    a = xb - fi
    fi = np.fmin(np.fmax(fi, f32(-2)), f32(n) + ONE)
    i = fi.astype(np.int64)
    return a, [np.clip(i + k, 0, n - 1) for k in (-1, 0, 1, 2)]


def tap(img, x, y, filt):
    """the tap of an (h, w, C) float32 image at texture coordinates (x, y) (texel i at i + 0.5) under filter `filt`:
    chain_ref.tap for BILINEAR, the cubic tap above otherwise"""
    if filt == BILINEAR:
        return C.tap(img, x, y)
    h, w = img.shape[:2]
    with np.errstate(all="ignore"):
        a, cols = _axis(w, x)
        b, rows = _axis(h, y)
        wx = [t[..., None] for t in weights(a, filt)]
        wy = [t[..., None] for t in weights(b, filt)]
        value = None
        for m in range(4):
            r = rows[m]
            row = ((wx[0] * img[r, cols[0]] + wx[1] * img[r, cols[1]]) + wx[2] * img[r, cols[2]]) + wx[3] * img[r, cols[3]]
            value = wy[0] * row if m == 0 else value + wy[m] * row
    assert value.dtype == f32
    return value


def _tap_under(filt):
    return lambda img, x, y: tap(img, x, y, filt)


def canvas_taps(ext0, ext1, ex, maps, filt):
    """[(c0, c1)] of the samples: the taps of the two canvases at (map + ex) + 0.5, each (out_h, out_w, 3) float32"""
    return C.plates(ext0[..., :3], ext1[..., :3], maps, ex, _tap_under(filt))


def canvas_mean(ext0, ext1, ex, maps, color_fa, color_from, filt, taps=None):
    """acc / (float)N of the canvas taps on the samples' maps, NOT clamped: (out_h, out_w, 3) float32 (taps: canvas_taps
    of the same arguments, for a test that blends them several ways)"""
    return C.blended_mean(canvas_taps(ext0, ext1, ex, maps, filt) if taps is None else taps, maps, color_fa, color_from)


def render_viewport_bytes(ext0, ext1, ex, maps, color_fa, color_from, filt, taps=None):
    """vm_frame_render_viewport_filtered on the maps of viewport_ref.sample_maps: (out_h, out_w, 3) uint8, the cubic filters'
    mean clamped to [0, 255] first (for BILINEAR defined where chain_ref.founded(maps) holds)"""
    return C.bytes_of(canvas_mean(ext0, ext1, ex, maps, color_fa, color_from, filt, taps), filt in CUBIC)


def layer_taps(layer0, layer1, maps, filt, lex=0):
    """[(c0, c1)] of the samples: the taps of the two layers at (map + lex) + 0.5, each (out_h, out_w, C) float32"""
    return C.plates(layer0, layer1, maps, lex, _tap_under(filt))


def layers_on_maps(layer0, layer1, maps, color_fa, color_from, filt, lex=0, taps=None):
    """vm_frame_render_viewport_filtered_layers on the maps of viewport_ref.sample_maps, unclamped: float32 (out_h, out_w) or
    (out_h, out_w, C) as the layers are.  lex: where the image begins in the layers' grid (0 tight; the frame's ex for what
    vm_frame_download_layers_ext hands out).  taps: layer_taps of the same arguments"""
    taps = layer_taps(layer0, layer1, maps, filt, lex) if taps is None else taps
    return C.like(C.blended_mean(taps, maps, color_fa, color_from), layer0)


def overshoot_case(w, h):
    """the case that tests the clamp: (rgb, v, viewport tuple) of a vertical 0 / 255 step plate, a zero field and the
    viewport {0.25, 0.25, 1, 1, w - 1, h - 1, 1, 1} -- every sample a quarter pixel behind a texel in x and y, so that the
    columns next to the step overshoot under Catmull-Rom and Mitchell"""
    rgb = np.zeros((h, w, 3), np.uint8)
    rgb[:, w // 2:] = 255
    return rgb, np.zeros((h, w, 2), f32), (0.25, 0.25, 1.0, 1.0, w - 1, h - 1, 1, 1)
