"""Viewports of the morph (include/vmorph.h: vm_viewport): where an output grid of any size lies over the
halfway domain, and how many sub-samples every output pixel takes.  Coordinates are pixel-EDGE: field pixel i covers
[i, i + 1), its centre is i + 0.5.  A Viewport is a value; the constructors below cover what a viewer, a proxy pipeline and
a delivery need, `validate` mirrors the checks of the C-ABI, and morph.Frame.render_viewport* take one.

    Viewport.identity(w, h)                         the frame itself: the bits of render_halfway
    Viewport.crop(x, y, w, h)                       a w x h window at native scale with its corner at (x, y)
    Viewport.fit(w, h, out_w, out_h)                the whole frame at another size
    Viewport.zoom(cx, cy, factor, out_w, out_h)     an out_w x out_h window centred on (cx, cy), `factor` times enlarged
    Viewport.overscan(w, h, margin)                 the frame and `margin` pixels beyond every edge
    .supersampled(nx, ny=None)                      the same viewport with nx x ny sub-samples per pixel
"""
import math

import numpy as np

from . import capi

MAX_SIDE = 32768
MAX_SAMPLES = 64


class Viewport:
    __slots__ = ("x0", "y0", "step_x", "step_y", "out_w", "out_h", "nx", "ny")

    def __init__(self, x0, y0, step_x, step_y, out_w, out_h, nx=1, ny=1):
        self.x0, self.y0, self.step_x, self.step_y = x0, y0, step_x, step_y
        self.out_w, self.out_h, self.nx, self.ny = out_w, out_h, nx, ny

    @classmethod
    def identity(cls, w, h):
        return cls(0.0, 0.0, 1.0, 1.0, w, h)

    @classmethod
    def crop(cls, x, y, w, h):
        return cls(x, y, 1.0, 1.0, w, h)

    @classmethod
    def fit(cls, w, h, out_w, out_h):
        return cls(0.0, 0.0, w / out_w, h / out_h, out_w, out_h)

    @classmethod
    def zoom(cls, cx, cy, factor, out_w, out_h):
        step = 1.0 / factor
        return cls(cx - 0.5 * out_w * step, cy - 0.5 * out_h * step, step, step, out_w, out_h)

    @classmethod
    def overscan(cls, w, h, margin):
        return cls(-float(margin), -float(margin), 1.0, 1.0, w + 2 * margin, h + 2 * margin)

    def supersampled(self, nx, ny=None):
        return Viewport(self.x0, self.y0, self.step_x, self.step_y, self.out_w, self.out_h, nx, nx if ny is None else ny)

    def astuple(self):
        return tuple(getattr(self, k) for k in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, Viewport) and self.astuple() == other.astuple()

    def __repr__(self):
        return "Viewport(x0=%r, y0=%r, step_x=%r, step_y=%r, out_w=%r, out_h=%r, nx=%r, ny=%r)" % self.astuple()

    def validate(self):
        """what the C-ABI answers VM_E_INVALID for, judged on the float32 / int values the call would receive: raises
        ValueError, returns self"""
        with np.errstate(over="ignore"):
            x0, y0, sx, sy = (float(np.float32(v)) for v in (self.x0, self.y0, self.step_x, self.step_y))
        if not (math.isfinite(x0) and math.isfinite(y0)):
            raise ValueError("viewport corner (%r, %r) is not finite" % (self.x0, self.y0))
        if not (math.isfinite(sx) and math.isfinite(sy) and sx > 0 and sy > 0):
            raise ValueError("viewport step (%r, %r) (finite, > 0)" % (self.step_x, self.step_y))
        for v in (self.out_w, self.out_h, self.nx, self.ny):
            if int(v) != v:
                raise ValueError("viewport sizes and sample counts are integers: %r" % (v,))
        if not (1 <= self.out_w <= MAX_SIDE and 1 <= self.out_h <= MAX_SIDE):
            raise ValueError("output of %r x %r (1..%d each)" % (self.out_w, self.out_h, MAX_SIDE))
        if self.nx < 1 or self.ny < 1 or self.nx * self.ny > MAX_SAMPLES:
            raise ValueError("%r x %r sub-samples (each >= 1, 1..%d together)" % (self.nx, self.ny, MAX_SAMPLES))
        return self

    def struct(self):
        """the vm_viewport the C-ABI takes (not validated: the library checks for itself)"""
        return capi.ViewportStruct(self.x0, self.y0, self.step_x, self.step_y, int(self.out_w), int(self.out_h),
                                   int(self.nx), int(self.ny))
