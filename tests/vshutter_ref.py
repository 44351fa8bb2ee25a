"""The float32 numpy statement of what videomorphing_amd/csrc/vm_vshutter.hip computes (include/vmorph.h): a
viewport of the morph over a shutter, uniformly and under a transition schedule.  Composed from the statements that
exist -- viewport_ref.sample_points and landing, the shutters' sample_times, transit_shutter_ref's rate planes and its
walk from q, and the tail of tests/chain_ref.py.  T = samples, N = nx * ny; time sample tau = 0 .. T - 1 is the OUTER
loop, sub-sample s = j * nx + i the INNER one, i fastest:

    f_tau = ((float)tau + 0.5f) / (float)T
    q     = viewport_ref.sample_points' (qx, qy) for (X, Y, i, j)
    uniform:    t_tau = fminf(fmaxf(geo_open + (geo_close - geo_open) * f_tau, 0), 1)
                (p, V) = the chain from q at geo_fa = t_tau;  c = blend(taps, color_fa, color_from)
    scheduled:  K = ramp(schedule_colour, t_color, ease)                once per call
                t_tau = t_open + (t_close - t_open) * f_tau             not clamped: ramp clamps per texel
                (p, V) = the chain from q under G_tau = ramp(schedule_geometry, t_tau, ease), g = tapr(G_tau, p) at every p
                k = tapr(K, p);  c = blend(taps, k, color_from)
    acc = acc + c                                                       from +0, in loop order
    result = acc / (float)(T * N); RGB8: (uint8)((double)result + 0.5)

A viewport is viewport_ref's tuple.  tests/test_vshutter_ref.py pins the statement to viewport_ref, shutter_ref and
transit_shutter_ref without a GPU; tests/test_gpu_viewport_shutter.py holds the kernels to it bit for bit."""
import chain_ref as C
import shutter_ref
import transit_shutter_ref as TS
import viewport_ref

MAX_CHAINS = 256        # samples * nx * ny of one call, at most (include/vmorph.h)


def _count(n, vp):
    assert 1 <= n <= shutter_ref.MAX_SAMPLES and n * vp[6] * vp[7] <= MAX_CHAINS


def uniform_maps(v, u, geo_open, geo_close, n, vp):
    """[(map0, map1)] of the T * N samples in loop order, each (out_h, out_w, 2)"""
    _count(n, vp)
    pts = viewport_ref.sample_points(vp)
    return [viewport_ref.landing(v, u, t, qx, qy) for t in shutter_ref.sample_times(geo_open, geo_close, n) for qx, qy in pts]


def scheduled_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease, vp):
    """[(map0, map1, k)] of the T * N samples in loop order (a schedule None: uniform (0, 1))"""
    _count(n, vp)
    Gs, K = TS.planes(v, sched_geo, sched_color, t_open, t_close, n, t_color, ease)
    pts = viewport_ref.sample_points(vp)
    return [TS.walk(v, u, G, K, q) for G in Gs for q in pts]


def bytes_on_maps(ext0, ext1, ex, maps, color_from, color_fa=None):
    """the RGB8 result on given sample maps of either family (defined where chain_ref.founded(maps) holds); a sample
    under a schedule is blended with its own k, the others with color_fa"""
    return C.bytes_of(shutter_ref.canvas_mean(ext0, ext1, ex, maps, color_fa, color_from))


def layers_on_maps(layer0, layer1, maps, color_from, color_fa=None):
    """the layer result on given sample maps: float32 (out_h, out_w) or (out_h, out_w, C) as the layers are"""
    return shutter_ref.layers_on_maps(layer0, layer1, maps, color_fa, color_from)


def render_viewport_shutter_bytes(ext0, ext1, ex, v, u, color_fa, geo_open, geo_close, n, color_from, vp):
    """vm_render_viewport_shutter: (out_h, out_w, 3) uint8"""
    return bytes_on_maps(ext0, ext1, ex, uniform_maps(v, u, geo_open, geo_close, n, vp), color_from, color_fa)


def render_viewport_transition_shutter_layers(layer0, layer1, v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease,
                                              color_from, vp):
    """vm_render_viewport_transition_shutter_layers"""
    maps = scheduled_maps(v, u, sched_geo, sched_color, t_open, t_close, n, t_color, ease, vp)
    return layers_on_maps(layer0, layer1, maps, color_from)
