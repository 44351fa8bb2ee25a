"""The float32 numpy statement of a shutter under a transition schedule (include/vmorph.h): what
videomorphing_amd/csrc/vm_tshutter.hip computes.  With ramp and tapr of tests/transit_ref.py, the taps and the blend of
tests/warp_ref.py and the mean of tests/shutter_ref.py, for N = samples:

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

walk() is the 20-round chain on given (G, K) planes: transit_ref.transition_maps ramps both planes at one time, and here
they belong to different times.  tests/test_transit_shutter_ref.py pins the statement to transit_ref and shutter_ref
without a GPU; tests/test_gpu_transition_shutter.py holds the kernels to it bit for bit."""
import numpy as np

import shutter_ref
import transit_ref
import warp_ref as R

f32 = np.float32
HALF, ONE = R.HALF, R.ONE
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


def walk(v, u, G, K):
    """(map0, map1, k) of the chain under the (h, w) rate planes G and K: transit_ref.transition_maps' rounds"""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    with np.errstate(all="ignore"):
        qy, qx = np.mgrid[0:h, 0:w].astype(f32)
        px, py = qx.copy(), qy.copy()
        V, U = R.tap(v, px + HALF, py + HALF), R.tap(u, px + HALF, py + HALF)
        g = transit_ref.tapr(G, px + HALF, py + HALF)
        for _ in range(R.ITERS):
            s1 = f32(2) * g - ONE
            s2 = f32(4) * g - f32(4) * g * g
            px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
            py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
            V = R.ALPHA * R.tap(v, px + HALF, py + HALF) + (ONE - R.ALPHA) * V
            U = R.ALPHA * R.tap(u, px + HALF, py + HALF) + (ONE - R.ALPHA) * U
            g = transit_ref.tapr(G, px + HALF, py + HALF)
        k = transit_ref.tapr(K, px + HALF, py + HALF)
        map0 = np.stack([px - V[..., 0], py - V[..., 1]], -1)
        map1 = np.stack([px + V[..., 0], py + V[..., 1]], -1)
    assert map0.dtype == f32 and map1.dtype == f32 and k.dtype == f32
    return map0, map1, k


def _plane(sched, w, h):
    return transit_ref.uniform_schedule(w, h) if sched is None else np.asarray(sched, dtype=f32)


def sample_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease):
    """[(map0, map1, k)] of the n samples (a schedule None: uniform (0, 1))"""
    h, w = np.asarray(v).shape[:2]
    sg, K = _plane(sched_geo, w, h), transit_ref.ramp(_plane(sched_color, w, h), t_color, ease)
    return [walk(v, u, transit_ref.ramp(sg, t, ease), K) for t in sample_times(t_open, t_close, n)]


def founded(maps):
    """where every sample's two positions are finite: where an RGB8 byte is defined"""
    return shutter_ref.founded([m[:2] for m in maps])


def canvas_mean(ext0, ext1, ex, maps, color_from):
    """acc / (float)N of the canvas taps on the samples' maps, blended with their k: (h, w, 3) float32"""
    e0, e1, exf = ext0[..., :3].astype(f32), ext1[..., :3].astype(f32), f32(ex)
    colours = []
    with np.errstate(all="ignore"):
        for m0, m1, k in maps:
            c0 = R.tap(e0, (m0[..., 0] + exf) + HALF, (m0[..., 1] + exf) + HALF)
            c1 = R.tap(e1, (m1[..., 0] + exf) + HALF, (m1[..., 1] + exf) + HALF)
            colours.append(R.blend(c0, c1, k[..., None], color_from))
    return shutter_ref._mean(colours, len(maps))


def layers_on_maps(layer0, layer1, maps, color_from):
    """the layer result on given sample maps (a test that needs several channel counts walks the chain once)"""
    l0, l1 = np.asarray(layer0, dtype=f32), np.asarray(layer1, dtype=f32)
    shape = l0.shape
    if l0.ndim == 2:
        l0, l1 = l0[..., None], l1[..., None]
    colours = []
    with np.errstate(all="ignore"):
        for m0, m1, k in maps:
            c0 = R.tap(l0, m0[..., 0] + HALF, m0[..., 1] + HALF)
            c1 = R.tap(l1, m1[..., 0] + HALF, m1[..., 1] + HALF)
            colours.append(R.blend(c0, c1, k[..., None], color_from))
    return shutter_ref._mean(colours, len(maps)).reshape(shape)


def render_bytes(ext0, ext1, ex, v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease, color_from):
    """vm_render_transition_shutter: (h, w, 3) uint8 (defined where founded(sample_maps(...)) holds)"""
    maps = sample_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease)
    return shutter_ref.bytes_of(canvas_mean(ext0, ext1, ex, maps, color_from))


def render_layers(layer0, layer1, v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease, color_from):
    """vm_render_transition_shutter_layers: float32 of the layers' shape"""
    return layers_on_maps(layer0, layer1, sample_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease), color_from)
