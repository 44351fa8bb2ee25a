"""Band tables of the multiband render calls (include/vmorph.h: vm_bands): how many times the two warped
plates and the colour weight are reduced, and how much every band's weight plane is sharpened about 0.5 before the band is
blended.  Band 0 is the finest, band `levels` the low-pass residual.  A Bands is a value; morph.Frame.render_multiband*
take one.

    Bands.linear(levels)                 all ones: the Burt-Adelson spline with the colour weight as its mask
    Bands.sharpen(levels, finest)        finest ** ((levels - l) / levels) on band l, 1 on the residual: detail switches
                                         in the middle 1 / finest of the transition, the colour dissolves over all of it
    Bands.for_size(w, h, most=5)         the deepest linear table whose coarsest level is still at least 2 x 2
"""
import numpy as np

from . import capi

MAX_LEVELS = capi.MULTIBAND_MAX_LEVELS


def level_sizes(w, h, levels):
    """[(w_l, h_l)] for l = 0..levels: w_(l+1) = (w_l + 1) // 2"""
    out = [(int(w), int(h))]
    for _ in range(levels):
        w, h = (out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2
        out.append((w, h))
    return out


class Bands:
    __slots__ = ("sharp",)

    def __init__(self, sharp):
        """sharp[0..levels]: one float32 per band"""
        self.sharp = tuple(float(np.float32(s)) for s in sharp)

    @property
    def levels(self):
        return len(self.sharp) - 1

    @classmethod
    def linear(cls, levels):
        return cls([1.0] * (int(levels) + 1))

    @classmethod
    def sharpen(cls, levels, finest):
        levels = int(levels)
        return cls([float(finest) ** ((levels - l) / levels) for l in range(levels)] + [1.0])

    @classmethod
    def for_size(cls, w, h, most=5):
        levels = 0
        while levels < min(int(most), MAX_LEVELS) and min(level_sizes(w, h, levels + 1)[-1]) >= 2:
            levels += 1
        return cls.linear(levels)

    def validate(self, w=None, h=None):
        """the checks of the C-ABI (ValueError); with a frame size, the coarsest level too"""
        if not 1 <= self.levels <= MAX_LEVELS:
            raise ValueError("%d levels (1..%d)" % (self.levels, MAX_LEVELS))
        if not all(np.isfinite(s) and s >= 1 for s in self.sharp):
            raise ValueError("sharp %r (finite, >= 1)" % (self.sharp,))
        if w is not None and min(level_sizes(w, h, self.levels)[-1]) < 2:
            raise ValueError("%d levels leave a %d x %d frame a coarsest level below 2 x 2" % (self.levels, w, h))
        return self

    def struct(self):
        """the vm_bands of this table (a table deeper than the struct holds is cut: the library refuses its level count)"""
        s = capi.BandsStruct()
        s.levels = self.levels
        for l, v in enumerate(self.sharp[:MAX_LEVELS + 1]):
            s.sharp[l] = v
        return s

    def __repr__(self):
        return "Bands(%r)" % (list(self.sharp),)
