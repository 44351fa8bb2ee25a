"""The float32 numpy statement of what videomorphing_amd/csrc/vm_shutter.hip computes: the compositor's chain
(tests/warp_ref.py: sampling_maps, tap, blend) walked at the N sample times of a shutter, the samples' colours summed in
float32 in sample order from +0 and divided by (float)N once.  For s = 0 .. N - 1:

    f   = ((float)s + 0.5f) / (float)N
    t_s = fminf(fmaxf(geo_open + (geo_close - geo_open) * f, 0), 1)
    c_s = blend(tap(side 0 at map0_s), tap(side 1 at map1_s), color_fa, color_from)      at geo_fa = t_s
    acc = acc + c_s

RGB8 from the extended canvases is (uint8)((double)(acc / (float)N) + 0.5) with the renderer's taps ((map + ex) + 0.5),
layers are acc / (float)N.  Every scalar is a float32 and every expression stands in the kernels' order (they are built
without contraction); numpy's float32 division is IEEE, as the kernels' is.  tests/test_shutter_ref.py pins the
statement to warp_ref without a GPU, tests/test_gpu_shutter.py holds the kernels to it bit for bit."""
import numpy as np

import warp_ref

f32 = np.float32
HALF = f32(0.5)
MAX_SAMPLES = 64


def sample_times(geo_open, geo_close, n):
    """the n times of the shutter, each clamped to [0, 1]: (n,) float32"""
    assert 1 <= n <= MAX_SAMPLES
    o, c = f32(geo_open), f32(geo_close)
    out = np.empty(n, f32)
    for s in range(n):
        f = (f32(s) + HALF) / f32(n)
        out[s] = np.fmin(np.fmax(o + (c - o) * f, f32(0)), f32(1))
    return out


def sample_maps(v, u, geo_open, geo_close, n):
    """[(map0, map1)] of the n samples"""
    return [warp_ref.sampling_maps(v, u, t)[:2] for t in sample_times(geo_open, geo_close, n)]


def founded(maps):
    """where every sample's two positions are finite: where an RGB8 byte is defined"""
    ok = True
    for m0, m1 in maps:
        ok = ok & np.isfinite(m0).all(-1) & np.isfinite(m1).all(-1)
    return ok


def _mean(colours, n):
    with np.errstate(all="ignore"):
        acc = np.zeros(colours[0].shape, f32)
        for c in colours:
            acc = acc + c
        out = acc / f32(n)
    assert out.dtype == f32
    return out


def canvas_mean(ext0, ext1, ex, maps, color_fa, color_from):
    """acc / (float)N of the canvas taps on the samples' maps: (h, w, 3) float32"""
    e0, e1, exf = ext0[..., :3].astype(f32), ext1[..., :3].astype(f32), f32(ex)
    colours = []
    with np.errstate(all="ignore"):
        for m0, m1 in maps:
            c0 = warp_ref.tap(e0, (m0[..., 0] + exf) + HALF, (m0[..., 1] + exf) + HALF)
            c1 = warp_ref.tap(e1, (m1[..., 0] + exf) + HALF, (m1[..., 1] + exf) + HALF)
            colours.append(warp_ref.blend(c0, c1, color_fa, color_from))
    return _mean(colours, len(maps))


def bytes_of(mean):
    """the statement's tail: + 0.5 in double, truncation"""
    with np.errstate(all="ignore"):
        return (mean.astype(np.float64) + 0.5).astype(np.uint8)


def layers_on_maps(layer0, layer1, maps, color_fa, color_from):
    """the layer result on given sample maps (a test that needs several channel counts walks the chain once)"""
    l0, l1 = np.asarray(layer0, dtype=f32), np.asarray(layer1, dtype=f32)
    shape = l0.shape
    if l0.ndim == 2:
        l0, l1 = l0[..., None], l1[..., None]
    colours = []
    with np.errstate(all="ignore"):
        for m0, m1 in maps:
            c0 = warp_ref.tap(l0, m0[..., 0] + HALF, m0[..., 1] + HALF)
            c1 = warp_ref.tap(l1, m1[..., 0] + HALF, m1[..., 1] + HALF)
            colours.append(warp_ref.blend(c0, c1, color_fa, color_from))
    return _mean(colours, len(maps)).reshape(shape)


def render_shutter_bytes(ext0, ext1, ex, v, u, color_fa, geo_open, geo_close, n, color_from):
    """vm_render_shutter: (h, w, 3) uint8 (defined where founded(sample_maps(...)) holds)"""
    return bytes_of(canvas_mean(ext0, ext1, ex, sample_maps(v, u, geo_open, geo_close, n), color_fa, color_from))


def render_shutter_layers(layer0, layer1, v, u, color_fa, geo_open, geo_close, n, color_from):
    """vm_render_shutter_layers: float32 of the layers' shape"""
    return layers_on_maps(layer0, layer1, sample_maps(v, u, geo_open, geo_close, n), color_fa, color_from)
