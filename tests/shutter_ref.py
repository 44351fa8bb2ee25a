"""The float32 numpy statement of what videomorphing_amd/csrc/vm_shutter.hip computes: the compositor's chain
(tests/warp_ref.py: sampling_maps) walked at the N sample times of a shutter, the samples' colours summed in float32 in
sample order from +0 and divided by (float)N once (the tail of tests/chain_ref.py).  For s = 0 .. N - 1:

    f   = ((float)s + 0.5f) / (float)N
    t_s = fminf(fmaxf(geo_open + (geo_close - geo_open) * f, 0), 1)
    c_s = blend(tap(side 0 at map0_s), tap(side 1 at map1_s), color_fa, color_from)      at geo_fa = t_s
    acc = acc + c_s

RGB8 from the extended canvases is (uint8)((double)(acc / (float)N) + 0.5) with the renderer's taps ((map + ex) + 0.5),
layers are acc / (float)N.  Every scalar is a float32 and every expression stands in the kernels' order (they are built
without contraction); numpy's float32 division is IEEE, as the kernels' is.  tests/test_shutter_ref.py pins the
statement to warp_ref without a GPU, tests/test_gpu_shutter.py holds the kernels to it bit for bit."""
import numpy as np

import chain_ref as C
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


def canvas_mean(ext0, ext1, ex, maps, color_fa, color_from):
    """acc / (float)N of the canvas taps on the samples' maps: (h, w, 3) float32"""
    return C.sampled_mean(ext0[..., :3], ext1[..., :3], maps, color_fa, color_from, ex)


def layers_on_maps(layer0, layer1, maps, color_fa, color_from):
    """the layer result on given sample maps, whatever their grid (a test that needs several channel counts walks the
    chain once): float32 (h, w) or (h, w, C) as the layers are"""
    return C.like(C.sampled_mean(layer0, layer1, maps, color_fa, color_from), layer0)


def render_shutter_bytes(ext0, ext1, ex, v, u, color_fa, geo_open, geo_close, n, color_from):
    """vm_render_shutter: (h, w, 3) uint8 (defined where chain_ref.founded(sample_maps(...)) holds)"""
    return C.bytes_of(canvas_mean(ext0, ext1, ex, sample_maps(v, u, geo_open, geo_close, n), color_fa, color_from))


def render_shutter_layers(layer0, layer1, v, u, color_fa, geo_open, geo_close, n, color_from):
    """vm_render_shutter_layers: float32 of the layers' shape"""
    return layers_on_maps(layer0, layer1, sample_maps(v, u, geo_open, geo_close, n), color_fa, color_from)
