"""The two halves every render statement is made of, stated once in float32 numpy: the compositor's fixed-point chain
(kernel_render_halfway_image, render.cu:16-60; vm_chain.h / vm_chain_win.h) and the sample loop's tail
(vm_shutter_tail.h).  The family modules -- warp_ref, transit_ref, shutter_ref, transit_shutter_ref, viewport_ref,
vshutter_ref, filter_ref, carry_ref, the render tail of layer_ext_ref, the plates of multiband_ref -- compose them with
what is their own.

The chain from a point q, 20 rounds, g the rate (geo_fa, or a rate plane tapped at p in lerp form, anew at every p):

    p = q;  V = tap(v, p);  U = tap(u, p);  g = rate at p
    s1 = 2 g - 1;  s2 = 4 g - 4 g g;  p = (q - s1 V) - s2 U
    V = 0.8f tap(v, p) + (1 - 0.8f) V;  U likewise;  g = rate at p
    map0 = p - V;  map1 = p + V;  resid = fmaxf(|p.x - l.x|, |p.y - l.y|), l the p before the last round

The tail on the N sample maps of a call: tap side 0 at (map0 + offset) + 0.5 and side 1 at (map1 + offset) + 0.5, blend
(with the call's color_fa, or the sample's own k), sum in float32 in sample order from +0, divide by (float)N once; RGB8
is (uint8)((double)mean + 0.5), after a clamp to [0, 255] where the call has one.

Every scalar is a float32, every expression stands in the kernels' order (they are built without contraction), fmaxf /
fminf are np.fmax / np.fmin (a NaN loses), and (p + 0.5) - 0.5 is formed the way the kernels form it.  Plain helpers:
nothing here is collected."""
import collections

import numpy as np

f32 = np.float32
HALF, ONE = f32(0.5), f32(1)
ITERS = 20              # render.cu:29
ALPHA = f32(0.8)


# ---- the taps
def _texels(w, h, x, y):
    """the fractions (a, b) and the clamp-to-edge indices (i0, i1, j0, j1) of the four texels about the texture
    coordinates (x, y) of a w x h image (texel i at i + 0.5)"""
    xb, yb = x - HALF, y - HALF
    fi, fj = np.floor(xb), np.floor(yb)
    a, b = xb - fi, yb - fj
    fi = np.fmin(np.fmax(fi, f32(-1)), f32(w))
    fj = np.fmin(np.fmax(fj, f32(-1)), f32(h))
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    def clamp(i, n):        # np.clip on integers, without its wrapper's cost: these four are most of a walk's time
        return np.minimum(np.maximum(i, 0), n - 1)

    return a, b, clamp(i0, w), clamp(i0 + 1, w), clamp(j0, h), clamp(j0 + 1, h)


def tap(img, x, y):
    """tap2 of vm_render.hip on an (h, w, C) float32 image: (1-a)(1-b) t00 + a(1-b) t10 + (1-a)b t01 + ab t11 from left
    to right, per channel"""
    a, b, i0, i1, j0, j1 = _texels(img.shape[1], img.shape[0], x, y)
    w00, w10 = ((ONE - a) * (ONE - b))[..., None], (a * (ONE - b))[..., None]
    w01, w11 = ((ONE - a) * b)[..., None], (a * b)[..., None]
    return ((w00 * img[j0, i0] + w10 * img[j0, i1]) + w01 * img[j1, i0]) + w11 * img[j1, i1]


def tapr(plane, x, y):
    """an (h, w) float32 rate plane at the same texels, in lerp form: r0 = t00 + a (t10 - t00),
    r1 = t01 + a (t11 - t01), r = r0 + b (r1 - r0)"""
    a, b, i0, i1, j0, j1 = _texels(plane.shape[1], plane.shape[0], x, y)
    t00, t10, t01, t11 = plane[j0, i0], plane[j0, i1], plane[j1, i0], plane[j1, i1]
    r0 = t00 + a * (t10 - t00)
    r1 = t01 + a * (t11 - t01)
    return r0 + b * (r1 - r0)


# ---- the chain
Walk = collections.namedtuple("Walk", "px py lx ly V U g")      # p, the p before the last round, the damped V and U, the last g


def grid(w, h):
    """(qx, qy): the pixel centres of a w x h frame, each (h, w) float32"""
    qy, qx = np.mgrid[0:h, 0:w].astype(f32)
    return qx, qy


def rate_at(plane, c):
    """the rate plane tapped at the chain's p"""
    with np.errstate(all="ignore"):
        return tapr(plane, c.px + HALF, c.py + HALF)


def walk(v, u, qx, qy, rate):
    """the 20 rounds from the points (qx, qy) (any shape) on the field v and the path u ((h, w, 2) float32; u None: the
    no-path form -- a zero path stays zero through the rounds, and s2 * 0 is still subtracted, as the kernels do).  rate: a
    float32 scalar, or an (h, w) rate plane, tapped at p before the first round and after every round"""
    v = np.ascontiguousarray(v, dtype=f32)
    u = np.zeros(v.shape, f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    rate = np.asarray(rate, dtype=f32)
    at = (lambda px, py: tapr(rate, px + HALF, py + HALF)) if rate.ndim else (lambda px, py: rate[()])
    with np.errstate(all="ignore"):
        px, py = qx.copy(), qy.copy()
        V, U = tap(v, px + HALF, py + HALF), tap(u, px + HALF, py + HALF)
        g = at(px, py)
        for _ in range(ITERS):
            lx, ly = px, py
            s1 = f32(2) * g - ONE
            s2 = f32(4) * g - f32(4) * g * g
            px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
            py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
            V = ALPHA * tap(v, px + HALF, py + HALF) + (ONE - ALPHA) * V
            U = ALPHA * tap(u, px + HALF, py + HALF) + (ONE - ALPHA) * U
            g = at(px, py)
    assert px.dtype == f32 and py.dtype == f32 and V.dtype == f32 and U.dtype == f32 and g.dtype == f32
    return Walk(px, py, lx, ly, V, U, g)


def landing(c):
    """(map0, map1) = (p - V, p + V): where the two sides are sampled, each (..., 2)"""
    with np.errstate(all="ignore"):
        return (np.stack([c.px - c.V[..., 0], c.py - c.V[..., 1]], -1), np.stack([c.px + c.V[..., 0], c.py + c.V[..., 1]], -1))


def resid(c):
    """the move of the last round"""
    with np.errstate(all="ignore"):
        return np.fmax(np.abs(c.px - c.lx), np.abs(c.py - c.ly))


def inside_flags(map0, map1, w, h):
    """bit 0: 0 <= map0.x <= w - 1 and 0 <= map0.y <= h - 1; bit 1: the same for map1 (a NaN fails every comparison)"""
    with np.errstate(invalid="ignore"):
        def inside(m):
            return (f32(0) <= m[..., 0]) & (m[..., 0] <= f32(w - 1)) & (f32(0) <= m[..., 1]) & (m[..., 1] <= f32(h - 1))
        return (inside(map0).astype(np.uint8) | (inside(map1).astype(np.uint8) << 1)).astype(np.uint8)


# ---- the tail
def as3(img):
    """an image as (h, w, C) float32: a plane gets its one channel"""
    a = np.asarray(img, dtype=f32)
    return a[..., None] if a.ndim == 2 else a


def like(out, layer):
    """an (h, w, C) result in the form of the layer it was made from: (h, w) for a plane"""
    return out[..., 0] if np.asarray(layer).ndim == 2 else out


def plates(img0, img1, maps, offset=0, tap=tap):
    """[(c0, c1)] of the samples of `maps` ([(map0, map1, ...)]): the two images tapped at (map + offset) + 0.5, each
    (..., C) float32.  offset: where the image begins in the images' grid (ex for canvases, lex for layers, 0 for tight
    ones).  tap: the bilinear tap, or filter_ref.tap under a filter"""
    img0, img1, off = as3(img0), as3(img1), f32(offset)
    with np.errstate(all="ignore"):
        return [(tap(img0, (m[0][..., 0] + off) + HALF, (m[0][..., 1] + off) + HALF),
                 tap(img1, (m[1][..., 0] + off) + HALF, (m[1][..., 1] + off) + HALF)) for m in maps]


def blend(c0, c1, color_fa, color_from):
    """color_from 0: c0, 2: c1, 1: c0 * (1 - color_fa) + c1 * color_fa in float32"""
    col = f32(color_fa)
    if color_from == 0:
        return c0
    if color_from == 2:
        return c1
    with np.errstate(all="ignore"):
        return c0 * (ONE - col) + c1 * col


def blended_mean(taps, maps, color_fa, color_from):
    """acc / (float)N of the samples' plates (`taps`: plates of `maps`), each blended with its own k where the sample
    carries one ((map0, map1, k): a call under a schedule) and with the call's color_fa otherwise"""
    with np.errstate(all="ignore"):
        acc = np.zeros(taps[0][0].shape, f32)
        for (c0, c1), m in zip(taps, maps):
            acc = acc + blend(c0, c1, m[2][..., None] if len(m) == 3 else color_fa, color_from)
        out = acc / f32(len(taps))
    assert out.dtype == f32
    return out


def sampled_mean(img0, img1, maps, color_fa, color_from, offset=0):
    """the whole tail short of the bytes: the blended mean of the images' plates on `maps`"""
    return blended_mean(plates(img0, img1, maps, offset), maps, color_fa, color_from)


def blended(img0, img1, map0, map1, color_fa, color_from, offset=0):
    """the tail of a call with one sample and no sum: the two plates on (map0, map1), blended"""
    (c0, c1), = plates(img0, img1, [(map0, map1)], offset)
    out = blend(c0, c1, color_fa, color_from)
    assert out.dtype == f32
    return out


def founded(maps):
    """where every sample's two positions are finite: where an RGB8 byte is defined"""
    ok = True
    for m in maps:
        ok = ok & np.isfinite(m[0]).all(-1) & np.isfinite(m[1]).all(-1)
    return ok


def bytes_of(mean, clamp=False):
    """RGB8 of a mean: + 0.5 in double, truncation; clamp: the cubic filters' and the multiband calls' clamp to [0, 255]
    first (fminf(fmaxf(.)): a NaN becomes 0)"""
    with np.errstate(all="ignore"):
        if clamp:
            mean = np.fmin(np.fmax(mean, f32(0)), f32(255))
            assert mean.dtype == f32
        return (mean.astype(np.float64) + 0.5).astype(np.uint8)
