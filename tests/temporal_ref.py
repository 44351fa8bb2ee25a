"""CPU statement (numpy) of the temporal coherence path, the one the library runs on the GPU in
vm_temporal.hip and the oracle restates in C (oracle/vm_oracle_temporal.c), written from the text
of Algorithm/upsample.cu:

    contributions       temp_ref (:28-62): every pixel of the neighbouring page taps the two flows at
                        p -/+ v, lands at p_ref = p + 0.5 (f0 + f1) with v_ref = v + 0.5 (f1 - f0) and
                        adds v_ref * fa and fa to the <= 4 in-frame pixels around p_ref
    splat_fixed         those contributions summed as the library and the oracle sum them: each one
                        x 2^32, rounded to the nearest integer (ties to even), added in exact integers
    splat_f64           the same contributions summed with math.fsum: what the reference's own float
                        atomicAdd approximates in whatever order its threads arrive
    normalise           fixed point -> float, interpolate_temp_ref (:64-77)
    initialize_temp     kernel_initialize_temp (:190-211)
    smooth              (:80-111) mean of the weighted pixels of the 3x3 window
    fill_zeros_x        (:115-151) row fill of the pixels without weight
    temporal_fill       the in-between page of upsample() (:297-337)

Arrays are (h, w, 2) fields and flows and (h, w) scalars.  Every float expression of the reference is
formed in float32, its double sub-expressions (the literals 1.0 of the weight and of 1.0 / distance)
in float64 and rounded once, so that splat_fixed and everything after it agree with the oracle to the
last bit (tests/test_temporal_ref.py).

The bound between the two sums, per target pixel with n contributions and exact sum S:

    |from_fixed(acc) - S| <= n 2^-33 + |S| 2^-24

(half a unit of the 2^-32 grid per contribution, one rounding to float at the end).

NaN and infinite flows or vectors are out of scope: (int)floorf and llrint of a NaN are undefined in
the reference, the oracle and the library alike."""
import math

import numpy as np

F32 = np.float32
_ONE, _HALF, _ZERO = F32(1), F32(0.5), F32(0)
_SCALE = 4294967296.0


def tap2(img, x, y):
    """tex2D of a float2 texture, linear filter, clamp addressing, unnormalised coordinates
    (upsample.cu:227-233): img (h, w, 2), x / y float32 arrays -> (..., 2)"""
    h, w = img.shape[:2]
    xb, yb = x - _HALF, y - _HALF
    fi, fj = np.floor(xb), np.floor(yb)
    a, b = (xb - fi)[..., None], (yb - fj)[..., None]
    i = np.clip(fi, F32(-1), F32(w)).astype(np.int64)
    j = np.clip(fj, F32(-1), F32(h)).astype(np.int64)
    i0, i1 = np.clip(i, 0, w - 1), np.clip(i + 1, 0, w - 1)
    j0, j1 = np.clip(j, 0, h - 1), np.clip(j + 1, 0, h - 1)
    t00, t10, t01, t11 = img[j0, i0], img[j0, i1], img[j1, i0], img[j1, i1]
    r = (_ONE - a) * (_ONE - b) * t00 + a * (_ONE - b) * t10 + (_ONE - a) * b * t01 + a * b * t11
    assert r.dtype == F32
    return r


class Contributions:
    """what one temp_ref launch adds: flat arrays over (source pixel, footprint corner), the corners in
    the reference's loop order (y outer, x inner).  `inside` marks the corners within the frame: only
    those are added."""

    def __init__(self, v, f0, f1, ssim=None):
        v, f0, f1 = (np.ascontiguousarray(a, dtype=F32) for a in (v, f0, f1))
        h, w = v.shape[:2]
        py, px = np.mgrid[0:h, 0:w]
        p_x, p_y = px.astype(F32), py.astype(F32)
        a = tap2(f0, p_x - v[..., 0] + _HALF, p_y - v[..., 1] + _HALF)
        b = tap2(f1, p_x + v[..., 0] + _HALF, p_y + v[..., 1] + _HALF)
        self.tap0 = (p_x - v[..., 0], p_y - v[..., 1])      # where the two taps look (pixel units)
        self.tap1 = (p_x + v[..., 0], p_y + v[..., 1])
        prx, pry = p_x + _HALF * (a[..., 0] + b[..., 0]), p_y + _HALF * (a[..., 1] + b[..., 1])
        vrx, vry = v[..., 0] + _HALF * (b[..., 0] - a[..., 0]), v[..., 1] + _HALF * (b[..., 1] - a[..., 1])
        xx, yy = np.floor(prx).astype(np.int64), np.floor(pry).astype(np.int64)
        s = np.ones((h, w), np.float64) if ssim is None else np.asarray(ssim, dtype=F32).astype(np.float64)
        tx, ty, fa = [], [], []
        for dy in (0, 1):
            for dx in (0, 1):
                x, y = xx + dx, yy + dy
                ax, ay = np.abs(x.astype(F32) - prx), np.abs(y.astype(F32) - pry)
                assert ax.dtype == F32
                # ssim_fa*(1.0-abs((float)x-p_ref.x))*(1.0-abs((float)y-p_ref.y)): one double product
                fa.append((s * (1.0 - ax.astype(np.float64)) * (1.0 - ay.astype(np.float64))).astype(F32))
                tx.append(x)
                ty.append(y)
        self.w, self.h = w, h
        self.p_ref = (prx, pry)
        self.tx, self.ty, self.fa = (np.stack(q, -1).reshape(-1) for q in (tx, ty, fa))
        self.cx = (np.repeat(vrx.reshape(-1), 4) * self.fa).astype(F32)
        self.cy = (np.repeat(vry.reshape(-1), 4) * self.fa).astype(F32)
        self.inside = (self.tx >= 0) & (self.tx < w) & (self.ty >= 0) & (self.ty < h)
        self.target = np.where(self.inside, self.ty * w + self.tx, -1)
        # a footprint the frame cuts: some corner inside, some outside
        ins = self.inside.reshape(-1, 4)
        self.cut = np.repeat(ins.any(1) & ~ins.all(1), 4)

    def count(self):
        """contributions per target pixel (h, w)"""
        return np.bincount(self.target[self.inside], minlength=self.w * self.h).reshape(self.h, self.w)


def to_fixed(c):
    """float32 -> int64 at 2^32, round to nearest even (c * 2^32 is exact in double)"""
    return np.rint(np.asarray(c, dtype=F32).astype(np.float64) * _SCALE).astype(np.int64)


def from_fixed(acc):
    return (np.asarray(acc, dtype=np.int64).astype(np.float64) / _SCALE).astype(F32)


def splat_fixed(contribs, w, h):
    """the three accumulators (h, w, 3: v.x, v.y, weight) of one or more temp_ref launches"""
    acc = np.zeros((h * w, 3), np.int64)
    for c in contribs:
        t = c.target[c.inside]
        for k, q in enumerate((c.cx, c.cy, c.fa)):
            np.add.at(acc[:, k], t, to_fixed(q[c.inside]))
    return acc.reshape(h, w, 3)


def splat_f64(contribs, w, h):
    """the same contributions summed without fixed point (math.fsum: the exact sum, rounded once to
    double): (sums (h, w, 3) float64, contributions per pixel (h, w))"""
    t = np.concatenate([c.target[c.inside] for c in contribs])
    if not len(t):
        return np.zeros((h, w, 3), np.float64), np.zeros((h, w), np.int64)
    order = np.argsort(t, kind="stable")
    t = t[order]
    cuts = np.flatnonzero(np.diff(t)) + 1
    starts = np.concatenate([[0], cuts])
    out = np.zeros((h * w, 3), np.float64)
    for k, name in enumerate(("cx", "cy", "fa")):
        q = np.concatenate([getattr(c, name)[c.inside] for c in contribs]).astype(np.float64)[order]
        for tgt, part in zip(t[starts], np.split(q, cuts)):
            out[tgt, k] = math.fsum(part)
    n = np.bincount(t, minlength=h * w) if len(t) else np.zeros(h * w, np.int64)
    return out.reshape(h, w, 3), n.reshape(h, w)


def fixed_sum_bound(S, n):
    """n 2^-33 + |S| 2^-24"""
    return n[..., None] * 2.0 ** -33 + np.abs(S) * 2.0 ** -24


def normalise(acc):
    """interpolate_temp_ref: (v_cur (h, w, 2), weight (h, w))"""
    f = from_fixed(acc)
    wt = f[..., 2]
    has = wt > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.where(has[..., None], f[..., :2] / wt[..., None], f[..., :2]).astype(F32)
    return v, wt


def initialize_temp(v_src, fa, fb, ssim, temp_ref, temp_mask):
    """initialize_temp(lvl, i, dir) for one page: `temp_ref` / `temp_mask` are the page's arrays before
    the call (kernel_initialize_temp leaves temp.ref as it is where nothing landed); returns the new pair"""
    h, w = v_src.shape[:2]
    v, wt = normalise(splat_fixed([Contributions(v_src, fa, fb, ssim)], w, h))
    has = wt > 0
    return (np.where(has[..., None], v, np.asarray(temp_ref, dtype=F32)).astype(F32),
            np.where(has, wt, _ZERO).astype(F32))


def _shift(a, dy, dx, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that is outside"""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def smooth(v_cur, weight):
    """v_out (pre-filled with zeros) = mean of v_cur over the pixels of the 3x3 window that have weight"""
    has = weight > 0
    ww = np.zeros(weight.shape, F32)
    s = np.zeros(v_cur.shape, F32)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            m = _shift(has, dy, dx, False)
            ww = np.where(m, ww + _ONE, ww)
            s = np.where(m[..., None], s + _shift(v_cur, dy, dx, _ZERO), s)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((ww > 0)[..., None], s / ww[..., None], _ZERO).astype(F32)


def nearest_weighted(weight):
    """per pixel the column of the nearest pixel with weight in its row, to the left and to the right
    (-1 / w where there is none)"""
    h, w = weight.shape
    cols = np.broadcast_to(np.arange(w), (h, w))
    has = weight > 0
    left = np.maximum.accumulate(np.where(has, cols, -1), axis=1)
    right = np.minimum.accumulate(np.where(has, cols, w)[:, ::-1], axis=1)[:, ::-1]
    return left, right


def fill_zeros_x(v_out, weight):
    """a pixel without weight takes (v_left + v_right) / (1 / d_left + 1 / d_right) of the nearest
    weighted pixels of its row -- the numerator is not weighted (as written in the reference), so a
    hole with one neighbour takes v * d"""
    h, w = weight.shape
    cols = np.broadcast_to(np.arange(w), (h, w))
    left, right = nearest_weighted(weight)
    hole = ~(weight > 0)
    hl, hr = hole & (left >= 0), hole & (right < w)
    rows = np.broadcast_to(np.arange(h)[:, None], (h, w))
    ww = np.zeros((h, w), F32)
    s = np.zeros(v_out.shape, F32)
    with np.errstate(divide="ignore"):
        # ww += 1.0 / (pos.x - x): the sum in double, stored to the float ww
        ww = np.where(hl, (ww.astype(np.float64) + 1.0 / np.where(hl, cols - left, 1)).astype(F32), ww)
        s = np.where(hl[..., None], s + v_out[rows, np.clip(left, 0, w - 1)], s)
        ww = np.where(hr, (ww.astype(np.float64) + 1.0 / np.where(hr, right - cols, 1)).astype(F32), ww)
        s = np.where(hr[..., None], s + v_out[rows, np.clip(right, 0, w - 1)], s)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((ww > 0)[..., None], s / ww[..., None], v_out).astype(F32)


def temporal_accumulate(v_prev, f0_prev, f1_prev, v_next, b0_next, b1_next):
    """the two temp_ref launches of an in-between page (no ssim factor)"""
    return [Contributions(v_prev, f0_prev, f1_prev), Contributions(v_next, b0_next, b1_next)]


def temporal_fill(v_prev, f0_prev, f1_prev, v_next, b0_next, b1_next):
    """the in-between page of upsample(): (page, v_cur, weight).  fill_zeros_y (:153-189) only sets entries
    of the weight array that is freed right after it: no effect on the page."""
    h, w = v_prev.shape[:2]
    acc = splat_fixed(temporal_accumulate(v_prev, f0_prev, f1_prev, v_next, b0_next, b1_next), w, h)
    v_cur, weight = normalise(acc)
    return fill_zeros_x(smooth(v_cur, weight), weight), v_cur, weight
