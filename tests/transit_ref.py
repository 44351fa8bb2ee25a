"""The float32 numpy statement of transition control (include/vmorph.h): what the RATES instantiations of
videomorphing_amd/csrc/vm_warp.hip compute.  A schedule is a plane of (t0, t1) pairs in the halfway domain; ramp() turns
it into a rate plane at time t, tapr() samples a rate plane at a tap position of the chain in lerp form, and
transition_maps() is warp_ref.sampling_maps with the scalar geo_fa replaced by g = tapr(G, p), taken anew at every p.
Everything else -- the field taps, the inside flags, the layer and canvas tails -- is warp_ref's, with the per-pixel k in
the place of color_fa.  tests/test_transit_ref.py pins the statement to warp_ref without a GPU;
tests/test_gpu_transition.py holds the kernels to it bit for bit."""
import math

import numpy as np

import warp_ref as R

f32 = np.float32
HALF, ONE = R.HALF, R.ONE
EASE_LINEAR, EASE_SMOOTH = 0, 1


def uniform_schedule(w, h):
    """(0, 1) everywhere: what a NULL plane of vm_frame_upload_schedule stands for"""
    s = np.zeros((h, w, 2), f32)
    s[..., 1] = 1
    return s


def ramp(sched, t, ease):
    """the rate plane of an (h, w, 2) schedule at time t:
    d = t1 - t0;  s = d > 0 ? fminf(fmaxf((t - t0) / d, 0), 1) : (t >= t0 ? 1 : 0);  smooth: (s s)(3 - 2 s)"""
    sched = np.asarray(sched, dtype=f32)
    t, t0, t1 = f32(t), sched[..., 0], sched[..., 1]
    with np.errstate(all="ignore"):
        d = t1 - t0
        s = np.where(d > 0, np.fmin(np.fmax((t - t0) / d, f32(0)), ONE), np.where(t >= t0, ONE, f32(0)))
        if ease == EASE_SMOOTH:
            s = (s * s) * (f32(3) - f32(2) * s)
    assert ease in (EASE_LINEAR, EASE_SMOOTH) and s.dtype == f32
    return s


def tapr(plane, x, y):
    """an (h, w) float32 rate plane at texture coordinates (x, y): warp_ref.tap's indices and clamps, in lerp form
    r0 = t00 + a (t10 - t00), r1 = t01 + a (t11 - t01), r = r0 + b (r1 - r0)"""
    h, w = plane.shape
    xb, yb = x - HALF, y - HALF
    fi, fj = np.floor(xb), np.floor(yb)
    a, b = xb - fi, yb - fj
    fi = np.fmin(np.fmax(fi, f32(-1)), f32(w))
    fj = np.fmin(np.fmax(fj, f32(-1)), f32(h))
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, w - 1), np.clip(j0 + 1, 0, h - 1)
    i0, j0 = np.clip(i0, 0, w - 1), np.clip(j0, 0, h - 1)
    t00, t10, t01, t11 = plane[j0, i0], plane[j0, i1], plane[j1, i0], plane[j1, i1]
    r0 = t00 + a * (t10 - t00)
    r1 = t01 + a * (t11 - t01)
    return r0 + b * (r1 - r0)


def transition_maps(v, u, sched_geo, sched_color, t, ease):
    """(map0, map1, resid, flags, rates) of a frame with the field v, the path u (None: no path) and the two schedules
    (None: uniform) at time t; rates is (h, w, 2): (g, k) as they stand after round 20"""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    G = ramp(uniform_schedule(w, h) if sched_geo is None else sched_geo, t, ease)
    K = ramp(uniform_schedule(w, h) if sched_color is None else sched_color, t, ease)
    with np.errstate(all="ignore"):
        qy, qx = np.mgrid[0:h, 0:w].astype(f32)
        px, py = qx.copy(), qy.copy()
        V, U = R.tap(v, px + HALF, py + HALF), R.tap(u, px + HALF, py + HALF)
        g = tapr(G, px + HALF, py + HALF)
        for _ in range(R.ITERS):
            lx, ly = px, py
            s1 = f32(2) * g - ONE
            s2 = f32(4) * g - f32(4) * g * g
            px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
            py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
            V = R.ALPHA * R.tap(v, px + HALF, py + HALF) + (ONE - R.ALPHA) * V
            U = R.ALPHA * R.tap(u, px + HALF, py + HALF) + (ONE - R.ALPHA) * U
            g = tapr(G, px + HALF, py + HALF)
        k = tapr(K, px + HALF, py + HALF)
        map0 = np.stack([px - V[..., 0], py - V[..., 1]], -1)
        map1 = np.stack([px + V[..., 0], py + V[..., 1]], -1)
        resid = np.fmax(np.abs(px - lx), np.abs(py - ly))
    rates = np.stack([g, k], -1)
    assert map0.dtype == f32 and map1.dtype == f32 and resid.dtype == f32 and rates.dtype == f32
    return map0, map1, resid, R.inside_flags(map0, map1), rates


def render_layers(layer0, layer1, map0, map1, k, color_from):
    """warp_ref.render_layers with the (h, w) plane k in the place of color_fa"""
    return R.render_layers(layer0, layer1, map0, map1, k[..., None], color_from)


def render_bytes(ext0, ext1, ex, map0, map1, k, color_from):
    """warp_ref.render_bytes (the renderer's tail) with the (h, w) plane k in the place of color_fa"""
    return R.render_bytes(ext0, ext1, ex, map0, map1, k[..., None], color_from)


def two_halves(w, h):
    """the left half (0, 0.5), the right half (0.5, 1): at t = 0.5 the left has arrived and the right has not started"""
    s = np.empty((h, w, 2), f32)
    s[:, :w // 2] = (0.0, 0.5)
    s[:, w // 2:] = (0.5, 1.0)
    return s


def two_halves_columns(v, w):
    """(left, right): the output columns at least m = ceil(max|v.x|) + 2 from the seam, where no tap of the chain
    reaches a texel of the other half"""
    m = int(math.ceil(float(np.abs(v[..., 0]).max()))) + 2
    seam = w // 2
    return np.arange(0, seam - m), np.arange(seam + m, w)
