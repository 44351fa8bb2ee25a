"""The float32 numpy statement of what videomorphing_amd/csrc/vm_warp.hip computes: the fixed point of the compositor
(kernel_render_halfway_image, render.cu:16-60) with its two sampling positions kept, the move of its last round, the
inside flags, and float layers sampled at those positions.  The chain, the taps and the blend are stated in
tests/chain_ref.py (walk, tap, blend): every scalar is a float32, every expression stands in the kernels' order (they are
built without contraction), fmaxf / fminf are np.fmax / np.fmin (a NaN loses), and (px + 0.5) - 0.5 is formed the way
the kernels form it.  Here the chain starts from the pixel centres under one geo_fa.  tests/test_warp_ref.py pins the
statement to the renderer's verified arithmetic without a GPU (its maps, sampled on the extended canvases, give the
oracle's bytes); tests/test_gpu_layers.py holds the kernels to it bit for bit."""
import numpy as np

import chain_ref as C

f32 = np.float32


def sampling_maps(v, u, geo_fa):
    """(map0, map1, resid, flags) of a frame with the field v and the path u ((h, w, 2) float32; u None: the no-path
    form)"""
    h, w = np.shape(v)[:2]
    c = C.walk(v, u, *C.grid(w, h), f32(geo_fa))
    map0, map1 = C.landing(c)
    return map0, map1, C.resid(c), C.inside_flags(map0, map1, w, h)


def inside_flags(map0, map1):
    """chain_ref.inside_flags of the maps of a whole frame: w and h are their grid's"""
    h, w = map0.shape[:2]
    return C.inside_flags(map0, map1, w, h)


def render_layers(layer0, layer1, map0, map1, color_fa, color_from):
    """two (h, w) or (h, w, C) float32 layers sampled at (map + 0.5) on the layer itself (the edge texel repeats) and
    blended: float32 of the layers' shape"""
    return C.like(C.blended(layer0, layer1, map0, map1, color_fa, color_from), layer0)


def render_bytes(ext0, ext1, ex, map0, map1, color_fa, color_from):
    """the renderer's tail on the maps: the extended RGBA8 canvases sampled at (map + ex) + 0.5, blended, + 0.5 in
    double, truncated (render.cu:39-57) -> (h, w, 3) uint8"""
    return C.bytes_of(C.blended(ext0[..., :3], ext1[..., :3], map0, map1, color_fa, color_from, ex))


def field(kind, w, h, rng):
    """the fields of tests/test_gpu_parity.py::test_render_window_hard_cases, and the smooth one"""
    from videomorphing_amd import synth
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    if kind == "smooth":
        return synth.displacement(w, h).astype(f32)
    if kind == "rough":
        return (14.0 * rng.randn(h, w, 2)).astype(f32)
    if kind == "large":
        return np.stack([55.0 + 3.0 * np.sin(yy / 7.0), -38.0 + 2.0 * np.cos(xx / 9.0)], -1).astype(f32)
    if kind == "shear":
        return np.stack([0.9 * (yy - h / 2), 0.7 * (xx - w / 2)], -1).astype(f32)
    if kind == "outside":
        return np.stack([0.6 * (xx - w / 2) + 30.0 * np.sign(xx - w / 2), 0.8 * (yy - h / 2) + 20.0 * np.sign(yy - h / 2)], -1).astype(f32)
    assert kind == "nan"
    v = (3.0 * rng.randn(h, w, 2)).astype(f32)
    v[::13, ::11, 0] = np.nan
    v[5::17, 3::7, 1] = np.inf
    v[h // 2, w // 2] = (-np.inf, np.nan)      # a tile centre or close to one
    return v


def path(w, h, rng):
    return (2.5 * rng.randn(h, w, 2)).astype(f32)
