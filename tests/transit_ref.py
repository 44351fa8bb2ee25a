"""The float32 numpy statement of transition control (include/vmorph.h): what the RATES instantiations of
videomorphing_amd/csrc/vm_warp.hip compute.  A schedule is a plane of (t0, t1) pairs in the halfway domain; ramp() turns
it into a rate plane at time t, chain_ref.tapr samples a rate plane at a tap position of the chain in lerp form, and
transition_maps() is warp_ref.sampling_maps with the scalar geo_fa replaced by g = tapr(G, p), taken anew at every p:
chain_ref.walk under the plane G.  Everything else -- the field taps, the inside flags, the layer and canvas tails -- is
warp_ref's, with the per-pixel k in the place of color_fa.  tests/test_transit_ref.py pins the statement to warp_ref
without a GPU; tests/test_gpu_transition.py holds the kernels to it bit for bit."""
import math

import numpy as np

import chain_ref as C
import warp_ref

f32 = np.float32
ONE = C.ONE
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


def transition_maps(v, u, sched_geo, sched_color, t, ease):
    """(map0, map1, resid, flags, rates) of a frame with the field v, the path u (None: no path) and the two schedules
    (None: uniform) at time t; rates is (h, w, 2): (g, k) as they stand after round 20"""
    h, w = np.shape(v)[:2]
    G = ramp(uniform_schedule(w, h) if sched_geo is None else sched_geo, t, ease)
    K = ramp(uniform_schedule(w, h) if sched_color is None else sched_color, t, ease)
    c = C.walk(v, u, *C.grid(w, h), G)
    map0, map1 = C.landing(c)
    return map0, map1, C.resid(c), C.inside_flags(map0, map1, w, h), np.stack([c.g, C.rate_at(K, c)], -1)


def render_layers(layer0, layer1, map0, map1, k, color_from):
    """warp_ref.render_layers with the (h, w) plane k in the place of color_fa"""
    return warp_ref.render_layers(layer0, layer1, map0, map1, k[..., None], color_from)


def render_bytes(ext0, ext1, ex, map0, map1, k, color_from):
    """warp_ref.render_bytes (the renderer's tail) with the (h, w) plane k in the place of color_fa"""
    return warp_ref.render_bytes(ext0, ext1, ex, map0, map1, k[..., None], color_from)


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
