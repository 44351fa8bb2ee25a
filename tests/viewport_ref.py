"""The float32 numpy statement of what videomorphing_amd/csrc/vm_viewport.hip computes: the compositor's chain started
from the nx x ny sub-sample points of every pixel of an output grid laid over the halfway domain, the samples' colours
summed in float32 in sample order from +0 and divided by (float)N once.  A viewport is the tuple (x0, y0, step_x, step_y,
out_w, out_h, nx, ny) of include/vmorph.h's vm_viewport (pixel-EDGE coordinates: field pixel i covers [i, i + 1)).  For
output pixel (X, Y) and s = j * nx + i:

    fx = ((float)i + 0.5f) / (float)nx             fy = ((float)j + 0.5f) / (float)ny
    qx = (x0 + ((float)X + fx) * step_x) - 0.5f    qy = (y0 + ((float)Y + fy) * step_y) - 0.5f
    (p, V)_s = the chain from q                    c_s = blend(tap(side 0 at p - V), tap(side 1 at p + V))
    acc = acc + c_s

The chain from q is stated here, in tests/warp_ref.py's expressions (sampling_maps there is the case q = the pixel);
the taps, the blend, the mean and the rounding to bytes are warp_ref's and shutter_ref's own.  Every scalar is a float32
and every expression stands in the kernels' order (they are built without contraction).  tests/test_viewport_ref.py pins
the statement to warp_ref and the oracle without a GPU, tests/test_gpu_viewport.py holds the kernels to it bit for bit."""
import numpy as np

import shutter_ref
import warp_ref
from warp_ref import ALPHA, HALF, ITERS, ONE, f32, tap

MAX_SAMPLES = 64
NAN, INF = float("nan"), float("inf")
# viewports the C-ABI answers VM_E_INVALID for (videomorphing_amd.viewport.Viewport.validate raises for the same) ...
INVALID_VIEWPORTS = [
    (NAN, 0.0, 1.0, 1.0, 4, 4, 1, 1), (0.0, INF, 1.0, 1.0, 4, 4, 1, 1), (-INF, 0.0, 1.0, 1.0, 4, 4, 1, 1),
    (0.0, 0.0, NAN, 1.0, 4, 4, 1, 1), (0.0, 0.0, 1.0, INF, 4, 4, 1, 1), (0.0, 0.0, 0.0, 1.0, 4, 4, 1, 1),
    (0.0, 0.0, 1.0, -0.5, 4, 4, 1, 1), (0.0, 0.0, -0.0, 1.0, 4, 4, 1, 1), (1e39, 0.0, 1.0, 1.0, 4, 4, 1, 1),
    (0.0, 0.0, 1e-50, 1.0, 4, 4, 1, 1),              # (float32: inf, and 0)
    (0.0, 0.0, 1.0, 1.0, 0, 4, 1, 1), (0.0, 0.0, 1.0, 1.0, 4, 0, 1, 1), (0.0, 0.0, 1.0, 1.0, -3, 4, 1, 1),
    (0.0, 0.0, 1.0, 1.0, 32769, 4, 1, 1), (0.0, 0.0, 1.0, 1.0, 4, 32769, 1, 1), (0.0, 0.0, 1.0, 1.0, 4, 1 << 30, 1, 1),
    (0.0, 0.0, 1.0, 1.0, 4, 4, 0, 1), (0.0, 0.0, 1.0, 1.0, 4, 4, 1, 0), (0.0, 0.0, 1.0, 1.0, 4, 4, -1, -1),
    (0.0, 0.0, 1.0, 1.0, 4, 4, 65, 1), (0.0, 0.0, 1.0, 1.0, 4, 4, 9, 8), (0.0, 0.0, 1.0, 1.0, 4, 4, 1 << 16, 1 << 16),
    (0.0, 0.0, 1.0, 1.0, 4, 4, -8, -8),
]
# ... and the edges it takes
EDGE_VIEWPORTS = [
    (0.0, 0.0, 1.0, 1.0, 1, 1, 1, 1), (-1e6, 1e6, 1e-3, 50.0, 3, 2, 64, 1), (0.5, 0.5, 1.0, 1.0, 2, 2, 8, 8),
    (0.0, 0.0, 1.0, 1.0, 2, 2, 1, 64),
]


def sample_fractions(n):
    """((float)i + 0.5f) / (float)n for i = 0 .. n - 1: (n,) float32"""
    return ((np.arange(n).astype(f32) + HALF) / f32(n)).astype(f32)


def sample_points(vp):
    """[(qx, qy)] of the N samples in sample order, each an (out_h, out_w) float32 plane"""
    x0, y0, sx, sy = (f32(t) for t in vp[:4])
    out_w, out_h, nx, ny = vp[4:]
    assert nx >= 1 and ny >= 1 and nx * ny <= MAX_SAMPLES
    Y, X = np.mgrid[0:out_h, 0:out_w].astype(f32)
    pts = []
    with np.errstate(all="ignore"):
        for fy in sample_fractions(ny):
            for fx in sample_fractions(nx):
                qx = (x0 + (X + fx) * sx) - HALF
                qy = (y0 + (Y + fy) * sy) - HALF
                assert qx.dtype == f32 and qy.dtype == f32
                pts.append((qx, qy))
    return pts


def landing(v, u, geo_fa, qx, qy):
    """(map0, map1) of the chain started from the points (qx, qy): warp_ref.sampling_maps with q in the pixel's place (u
    None: the no-path form)"""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    geo = f32(geo_fa)
    with np.errstate(all="ignore"):
        s1 = f32(2) * geo - ONE
        s2 = f32(4) * geo - f32(4) * geo * geo
        px, py = qx.copy(), qy.copy()
        V, U = tap(v, px + HALF, py + HALF), tap(u, px + HALF, py + HALF)
        for _ in range(ITERS):
            px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
            py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
            V = ALPHA * tap(v, px + HALF, py + HALF) + (ONE - ALPHA) * V
            U = ALPHA * tap(u, px + HALF, py + HALF) + (ONE - ALPHA) * U
        map0 = np.stack([px - V[..., 0], py - V[..., 1]], -1)
        map1 = np.stack([px + V[..., 0], py + V[..., 1]], -1)
    assert map0.dtype == f32 and map1.dtype == f32
    return map0, map1


def sample_maps(v, u, geo_fa, vp):
    """[(map0, map1)] of the N samples, each (out_h, out_w, 2)"""
    return [landing(v, u, geo_fa, qx, qy) for qx, qy in sample_points(vp)]


founded = shutter_ref.founded


def render_viewport_bytes(ext0, ext1, ex, v, u, color_fa, geo_fa, color_from, vp, maps=None):
    """vm_render_viewport: (out_h, out_w, 3) uint8 (defined where founded(sample_maps(...)) holds)"""
    maps = sample_maps(v, u, geo_fa, vp) if maps is None else maps
    return shutter_ref.bytes_of(shutter_ref.canvas_mean(ext0, ext1, ex, maps, color_fa, color_from))


def render_viewport_layers(layer0, layer1, v, u, color_fa, geo_fa, color_from, vp, maps=None):
    """vm_render_viewport_layers: float32 (out_h, out_w) or (out_h, out_w, C) as the layers are"""
    maps = sample_maps(v, u, geo_fa, vp) if maps is None else maps
    return layers_on_maps(layer0, layer1, maps, color_fa, color_from)


def layers_on_maps(layer0, layer1, maps, color_fa, color_from):
    """shutter_ref.layers_on_maps on an output grid that is not the layers' (its result takes the layers' shape)"""
    l0, l1 = np.asarray(layer0, dtype=f32), np.asarray(layer1, dtype=f32)
    flat = l0.ndim == 2
    if flat:
        l0, l1 = l0[..., None], l1[..., None]
    colours = []
    with np.errstate(all="ignore"):
        for m0, m1 in maps:
            c0 = tap(l0, m0[..., 0] + HALF, m0[..., 1] + HALF)
            c1 = tap(l1, m1[..., 0] + HALF, m1[..., 1] + HALF)
            colours.append(warp_ref.blend(c0, c1, color_fa, color_from))
    out = shutter_ref._mean(colours, len(maps))
    return out[..., 0] if flat else out
