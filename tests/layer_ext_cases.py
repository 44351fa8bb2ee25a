"""What tests/test_layer_ext_ref.py and tests/test_gpu_layer_ext.py share: the shapes, the fields, the layers and the
float64 statement's solutions (computed once per case, shared, never written).  Plain helpers: nothing here is
collected."""
import functools

import numpy as np

import layer_ext_ref as R
from render_cases import field as _field

f32 = np.float32

# (w, h, ex): two grids above the solver's one-workgroup tail with partial tiles (154 x 100 and 221 x 95), a hierarchy
# that is all tail (39 x 13), every clamp with three interior pixels (9 x 7)
SHAPES = [(138, 84, 8), (203, 77, 9), (33, 7, 3), (5, 3, 2)]
# render_cases.field's kinds, and constant power-of-two fields, whose chain lands on integers (0.8f and 1 - 0.8f times a
# power of two are exact)
KINDS = ["smooth", "large", "outside"]
CONSTANTS = {"right2": (2.0, 0.0), "left2": (-2.0, 0.0), "down4": (0.0, 4.0), "up4": (0.0, -4.0)}
CHANNELS = [1, 3, 4]


@functools.lru_cache(maxsize=None)
def field(w, h, kind):
    if kind == "zero":
        v = np.zeros((h, w, 2), f32)
    elif kind in CONSTANTS:
        v = np.empty((h, w, 2), f32)
        v[...] = CONSTANTS[kind]
    else:
        return _field(w, h, kind, False)[0]
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def layers(w, h, c, seed, scale=1.0):
    """two (h, w, c) float32 layers drawn in [0, scale]: smooth structure plus noise, so that the extension has gradients
    of every size"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = []
    for k in range(2):
        a = 0.5 + 0.25 * np.sin(xx / 5.0 + k)[..., None] * np.cos(yy[..., None] / 3.0 + np.arange(c))
        a = np.clip(a + 0.25 * (rng.rand(h, w, c) - 0.5), 0.0, 1.0) * scale
        a = a.astype(f32)
        a.setflags(write=False)
        out.append(a)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference(w, h, ex, kind, c, seed, scale=1.0):
    """((extended float64, type map) of side 1, the same of side 2) of the case's layers under its field"""
    l0, l1 = layers(w, h, c, seed, scale)
    v = field(w, h, kind)
    out = (R.extend(l0, l1, v, ex, 1), R.extend(l1, l0, v, ex, 2))
    for e, t in out:
        e.setflags(write=False)
        t.setflags(write=False)
    return out
