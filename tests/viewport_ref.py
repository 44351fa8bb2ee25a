"""The float32 numpy statement of what videomorphing_amd/csrc/vm_viewport.hip computes: the compositor's chain started
from the nx x ny sub-sample points of every pixel of an output grid laid over the halfway domain, the samples' colours
summed in float32 in sample order from +0 and divided by (float)N once.  A viewport is the tuple (x0, y0, step_x, step_y,
out_w, out_h, nx, ny) of include/vmorph.h's vm_viewport (pixel-EDGE coordinates: field pixel i covers [i, i + 1)).  For
output pixel (X, Y) and s = j * nx + i:

    fx = ((float)i + 0.5f) / (float)nx             fy = ((float)j + 0.5f) / (float)ny
    qx = (x0 + ((float)X + fx) * step_x) - 0.5f    qy = (y0 + ((float)Y + fy) * step_y) - 0.5f
    (p, V)_s = the chain from q                    c_s = blend(tap(side 0 at p - V), tap(side 1 at p + V))
    acc = acc + c_s

The chain from q is chain_ref.walk (warp_ref.sampling_maps is the case q = the pixel); the taps, the blend, the mean and
the rounding to bytes are chain_ref's tail, as shutter_ref composes it.  Every scalar is a float32 and every expression
stands in the kernels' order (they are built without contraction).  tests/test_viewport_ref.py pins
the statement to warp_ref and the oracle without a GPU, tests/test_gpu_viewport.py holds the kernels to it bit for bit."""
import numpy as np

import chain_ref as C
import shutter_ref
from chain_ref import HALF, f32

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
    return C.landing(C.walk(v, u, qx, qy, f32(geo_fa)))


def sample_maps(v, u, geo_fa, vp):
    """[(map0, map1)] of the N samples, each (out_h, out_w, 2)"""
    return [landing(v, u, geo_fa, qx, qy) for qx, qy in sample_points(vp)]


layers_on_maps = shutter_ref.layers_on_maps         # the same tail: its result takes the maps' grid and the layers' form


def render_viewport_bytes(ext0, ext1, ex, v, u, color_fa, geo_fa, color_from, vp, maps=None):
    """vm_render_viewport: (out_h, out_w, 3) uint8 (defined where chain_ref.founded(sample_maps(...)) holds)"""
    maps = sample_maps(v, u, geo_fa, vp) if maps is None else maps
    return C.bytes_of(shutter_ref.canvas_mean(ext0, ext1, ex, maps, color_fa, color_from))


def render_viewport_layers(layer0, layer1, v, u, color_fa, geo_fa, color_from, vp, maps=None):
    """vm_render_viewport_layers: float32 (out_h, out_w) or (out_h, out_w, C) as the layers are"""
    maps = sample_maps(v, u, geo_fa, vp) if maps is None else maps
    return layers_on_maps(layer0, layer1, maps, color_fa, color_from)
