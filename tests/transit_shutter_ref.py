"""The float32 numpy statement of a shutter under a transition schedule (include/vmorph.h): what
videomorphing_amd/csrc/vm_tshutter.hip computes.  With ramp of tests/transit_ref.py and the chain, the rate tap and the
tail of tests/chain_ref.py, for N = samples:

    K   = ramp(schedule_colour, t_color, ease)                 once per call
    for s = 0 .. N - 1:
      f   = ((float)s + 0.5f) / (float)N
      t_s = t_open + (t_close - t_open) * f                    not clamped: ramp clamps per texel
      G_s = ramp(schedule_geometry, t_s, ease)
      p_s, V_s = the 20 rounds under G_s, g = tapr(G_s, p) anew at every p
      k_s = tapr(K, p_s)
      c_s = blend(tap(side 0 at map0_s), tap(side 1 at map1_s), k_s, color_from)
      acc = acc + c_s
    result = acc / (float)N; RGB8: (uint8)((double)result + 0.5)

walk() is the chain on given (G, K) planes: transit_ref.transition_maps ramps both planes at one time, and here they
belong to different times.  tests/test_transit_shutter_ref.py pins the statement to transit_ref and shutter_ref without
a GPU; tests/test_gpu_transition_shutter.py holds the kernels to it bit for bit."""
import numpy as np

import chain_ref as C
import shutter_ref
import transit_ref

f32 = np.float32
HALF = f32(0.5)
MAX_SAMPLES = shutter_ref.MAX_SAMPLES


def sample_times(t_open, t_close, n):
    """the n times of the shutter, not clamped: (n,) float32"""
    assert 1 <= n <= MAX_SAMPLES
    o, c = f32(t_open), f32(t_close)
    out = np.empty(n, f32)
    with np.errstate(all="ignore"):
        for s in range(n):
            out[s] = o + (c - o) * ((f32(s) + HALF) / f32(n))
    return out


def walk(v, u, G, K, q=None):
    """(map0, map1, k) of the chain under the (h, w) rate planes G and K, started from the points q = (qx, qy) (None: the
    pixel centres)"""
    h, w = np.shape(v)[:2]
    c = C.walk(v, u, *(C.grid(w, h) if q is None else q), G)
    return C.landing(c) + (C.rate_at(K, c),)


def planes(v, sched_geo, sched_color, t_open, t_close, n, t_color, ease):
    """([G_s] of the n samples, K) (a schedule None: uniform (0, 1))"""
    h, w = np.shape(v)[:2]
    sg, sc = (transit_ref.uniform_schedule(w, h) if s is None else np.asarray(s, dtype=f32) for s in (sched_geo, sched_color))
    return [transit_ref.ramp(sg, t, ease) for t in sample_times(t_open, t_close, n)], transit_ref.ramp(sc, t_color, ease)


def sample_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease):
    """[(map0, map1, k)] of the n samples"""
    Gs, K = planes(v, sched_geo, sched_color, t_open, t_close, n, t_color, ease)
    return [walk(v, u, G, K) for G in Gs]


def canvas_mean(ext0, ext1, ex, maps, color_from):
    """acc / (float)N of the canvas taps on the samples' maps, blended with their k: (h, w, 3) float32"""
    return C.sampled_mean(ext0[..., :3], ext1[..., :3], maps, None, color_from, ex)


def layers_on_maps(layer0, layer1, maps, color_from):
    """the layer result on given sample maps (a test that needs several channel counts walks the chain once)"""
    return C.like(C.sampled_mean(layer0, layer1, maps, None, color_from), layer0)


def render_layers(layer0, layer1, v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease, color_from):
    """vm_render_transition_shutter_layers: float32 of the layers' shape"""
    return layers_on_maps(layer0, layer1, sample_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease), color_from)
