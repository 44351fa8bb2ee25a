"""CPU statement (numpy, float64 by default) of the pyramid builder's chain, the one the library runs on the
GPU in vm_pyramid.hip / vm_temporal.hip and the oracle restates in C (oracle/vm_oracle_pyramid.c):

    load / flow_load            bytes or flows -> three planes of linear light
    scale                       per axis, the axis with the larger reduction first:
        down_axis               normalised cubic B-spline gather, then the inverse of the sampled
                                B-spline [1/6 4/6 1/6] with mirror boundary along the same axis
        up_axis                 (also the same-size case) to gamma space, that inverse, cubic B-spline
                                reconstruction, back to linear light
    store_gray / flow_store     clamp, curve, luma weights or range and size ratio
    flow_concat                 f(p) += bilinear(f_next, p + f(p))

Arrays are (3, h, w) planes, (h, w) lumas and (h, w, 2) flows; every line of an axis is worked on at once.

Working precision: every function takes `dtype`.  With np.float32 every array and every intermediate is
float32 wherever the C code's is (its double sub-expressions stay double), so the result agrees with the
oracle to the last bits (tests/test_pyramid_ref.py).  With np.float64 the same real-valued function is
evaluated in double: the code's float constants (0.055f, 1.f / 2.4f, 1.f / 255.f, the size ratios ...) are
rounded to float32 once, as the code rounds them, and then widened.  dist(f(.., float32), f(..)) is the
yardstick of the GPU checks: what float32 arithmetic may differ by (tests/test_gpu_pyramid_stages.py)."""
import numpy as np

F32 = np.float32


def _c(v, dtype):
    """a float constant of the code: rounded to float32, held in the working precision"""
    return dtype(F32(v))


def _pow(f, e):
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.power(f, e)


def srgbcurve(f, dtype=np.float64):
    a = _c(0.055, dtype)
    one_a = dtype(F32(1) + F32(0.055))
    e = dtype(F32(1) / F32(2.4))
    return np.where(f <= _c(0.0031308, dtype), _c(12.92, dtype) * f, one_a * _pow(f, e) - a).astype(dtype)


def srgbuncurve(f, dtype=np.float64):
    a = _c(0.055, dtype)
    one_a = dtype(F32(1) + F32(0.055))
    return np.where(f <= _c(0.04045, dtype), f / _c(12.92, dtype), _pow((f + a) / one_a, _c(2.4, dtype))).astype(dtype)


def bspline3(r, dtype=np.float64):
    r = np.abs(np.asarray(r, dtype=dtype))
    two, three, four, six, eight, twelve = (dtype(v) for v in (2, 3, 4, 6, 8, 12))
    inner = (four + r * r * (-six + three * r)) / six
    outer = (eight + r * (-twelve + (six - r) * r)) / six
    return np.where(r < 1, inner, np.where(r < two, outer, dtype(0))).astype(dtype)


def ext_mirror(i, n):
    i = np.mod(i, 2 * n)                                   # the non-negative remainder: ext_repeat
    return np.where(i >= n, 2 * n - i - 1, i)


_FACTORS = {}


def tri_factor(n, dtype=np.float64):
    """(lower, inverse pivot, upper) of the LU factors, without pivoting, of the tridiagonal
    [B3(1) B3(0) B3(-1)] operator with mirror boundary on n samples: lower[j] = L(j, j - 1),
    upper[j] = U(j, j + 1)"""
    key = (n, np.dtype(dtype).name)
    if key in _FACTORS:
        return _FACTORS[key]
    kern = [dtype(bspline3(dtype(v), dtype)) for v in (1, 0, -1)]
    band = np.zeros((3, n), dtype=dtype)                   # A(i, i - 1), A(i, i), A(i, i + 1)
    for i in range(n):
        for k in range(3):
            j = int(ext_mirror(i + k - 1, n))              # at the two ends the mirror folds a tap back in
            band[j - i + 1, i] += kern[k]
    sub, dia, sup = band
    lower, inv = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    d = dia[0]
    for p in range(n):
        inv[p] = dtype(1) / d
        if p + 1 < n:
            lower[p + 1] = dtype(sub[p + 1] * inv[p])
            d = dtype(dia[p + 1] - dtype(lower[p + 1] * sup[p]))
    _FACTORS[key] = (lower, inv, sup)
    return _FACTORS[key]


def tri_solve(x, dtype=np.float64):
    """in place along the last axis of x (lines, n)"""
    n = x.shape[-1]
    lower, inv, upper = tri_factor(n, dtype)
    for j in range(1, n):
        x[..., j] -= lower[j] * x[..., j - 1]
    for j in range(n - 1, -1, -1):
        if j + 1 < n:
            x[..., j] -= upper[j] * x[..., j + 1]
        x[..., j] *= inv[j]
    return x


def down_axis(x, nout, dtype=np.float64):
    """the gather of a reduction along the last axis: (lines, nin) -> (lines, nout), before the solve"""
    nin = x.shape[-1]
    inv_sw = dtype(dtype(nout) * (dtype(1) / dtype(nin)))
    sw = dtype(1) / inv_sw
    half, s = dtype(0.5), dtype(4)
    o = np.arange(nout)
    of = o.astype(dtype)
    lo = np.ceil(half * sw * (dtype(2) * of + dtype(1) - s) - half).astype(np.int64)
    hi = np.floor(half * sw * (dtype(2) * of + dtype(1) + s) - half).astype(np.int64)
    none = lo > hi
    mid = np.trunc(half * sw * (dtype(2) * of + dtype(1))).astype(np.int64)
    lo, hi = np.where(none, mid, lo), np.where(none, mid, hi)
    acc = np.zeros(x.shape[:-1] + (nout,), dtype=dtype)
    acc_w = np.zeros(nout, dtype=dtype)
    for k in range(int((hi - lo).max()) + 1):
        i = lo + k
        prod = (i.astype(dtype) + half) * inv_sw
        kj = (0.5 + o.astype(np.float64) - prod.astype(np.float64)).astype(dtype)   # `0.5 + o - ...` is double there
        wgt = np.where(i <= hi, bspline3(kj, dtype), dtype(0)).astype(dtype)
        q = np.clip(ext_mirror(i, nin), 0, nin - 1)
        acc += x[..., q] * wgt
        acc_w += wgt
    return acc / acc_w


def up_axis(x, nout, dtype=np.float64):
    """the reconstruction along the last axis of prefiltered lines: (lines, nin) -> (lines, nout)"""
    nin = x.shape[-1]
    inv_sw = dtype(dtype(nin) * (dtype(1) / dtype(nout)))
    f = (np.arange(nout).astype(dtype) + dtype(0.5)) * inv_sw - dtype(0.5)
    c = np.floor(f).astype(np.int64)
    d = (f - c.astype(dtype)).astype(dtype)
    acc = np.zeros(x.shape[:-1] + (nout,), dtype=dtype)
    for j in range(-1, 3):
        q = np.clip(ext_mirror(c + j, nin), 0, nin - 1)
        acc += x[..., q] * bspline3(d - dtype(j), dtype)
    return acc


def scale_axis(img, nout, axis, dtype=np.float64):
    """one axis of (3, h, w) planes; axis 0 = along rows (x), 1 = along columns (y)"""
    x = img if axis == 0 else np.swapaxes(img, 1, 2)
    x = np.ascontiguousarray(x, dtype=dtype)
    nin = x.shape[-1]
    if nout < nin:
        out = tri_solve(np.ascontiguousarray(down_axis(x, nout, dtype)), dtype)
    else:
        out = srgbuncurve(up_axis(tri_solve(srgbcurve(x, dtype), dtype), nout, dtype), dtype)
    return out if axis == 0 else np.ascontiguousarray(np.swapaxes(out, 1, 2))


def columns_first(w, h, wout, hout):
    return hout * w < wout * h


def scale(img, wout, hout, dtype=np.float64):
    """(3, h, w) -> (3, hout, wout)"""
    img = np.asarray(img, dtype=dtype)
    _, h, w = img.shape
    if columns_first(w, h, wout, hout):
        return scale_axis(scale_axis(img, hout, 1, dtype), wout, 0, dtype)
    return scale_axis(scale_axis(img, wout, 0, dtype), hout, 1, dtype)


def load(rgb, dtype=np.float64):
    """(h, w, 3) uint8 -> (3, h, w) linear light"""
    tof = dtype(F32(1) / F32(255))
    return srgbuncurve(np.moveaxis(np.asarray(rgb), -1, 0).astype(dtype) * tof, dtype)


def store_gray(img, dtype=np.float64):
    c = srgbcurve(np.clip(np.asarray(img, dtype=dtype), 0, 1), dtype) * dtype(255)
    c = c.astype(np.float64)                               # the weights are double literals
    return (c[0] * 0.299 + c[1] * 0.587 + c[2] * 0.114).astype(dtype)


def luma_pyramid(rgb, nlevels, dtype=np.float64):
    """lumas of the levels 1..nlevels, finest first: same size, then ceil-halved"""
    img = load(rgb, dtype)
    _, h, w = img.shape
    out = []
    for el in range(nlevels):
        if el:
            w, h = (w + 1) // 2, (h + 1) // 2
        img = scale(img, w, h, dtype)
        out.append(store_gray(img, dtype))
    return out


FLOW_MIN, FLOW_MAX = -50.0, 50.0


def flow_load(flow, dtype=np.float64):
    flow = np.asarray(flow, dtype=dtype)
    mn = dtype(FLOW_MIN)
    tof = dtype(F32(1) / (F32(FLOW_MAX) - F32(FLOW_MIN)))
    rg = srgbuncurve((np.moveaxis(flow, -1, 0) - mn) * tof, dtype)
    return np.concatenate([rg, np.ones((1,) + flow.shape[:2], dtype=dtype)])


def flow_store(img, w_in, h_in, dtype=np.float64):
    """(3, hout, wout) -> (hout, wout, 2), x the size ratio when either side shrank"""
    _, hout, wout = img.shape
    mn, mx = dtype(FLOW_MIN), dtype(FLOW_MAX)
    f = srgbcurve(np.clip(np.asarray(img[:2], dtype=dtype), 0, 1), dtype) * (mx - mn) + mn
    ratio = (dtype(F32(wout) / F32(w_in)), dtype(F32(hout) / F32(h_in)))
    if ratio[0] < 1 or ratio[1] < 1:
        f = np.stack([f[0] * ratio[0], f[1] * ratio[1]])
    return np.ascontiguousarray(np.moveaxis(f, 0, -1).astype(dtype))


def flow_scale(flow, wout, hout, dtype=np.float64):
    h, w = np.asarray(flow).shape[:2]
    return flow_store(scale(flow_load(flow, dtype), wout, hout, dtype), w, h, dtype)


def flow_concat(f, f_next, dtype=np.float64):
    f, f_next = np.asarray(f, dtype=dtype), np.asarray(f_next, dtype=dtype)
    h, w = f.shape[:2]
    y, x = np.mgrid[0:h, 0:w]
    px, py = x.astype(dtype) + f[..., 0], y.astype(dtype) + f[..., 1]
    x0, y0 = np.floor(px), np.floor(py)
    x1, y1 = np.ceil(px), np.ceil(py)
    u, v = (px - x0)[..., None], (py - y0)[..., None]
    one = dtype(1)

    def tap(tx, ty):
        return f_next[np.clip(ty, 0, h - 1).astype(np.int64), np.clip(tx, 0, w - 1).astype(np.int64)]
    o = tap(x0, y0) * (one - u) * (one - v) + tap(x0, y1) * (one - u) * v + tap(x1, y0) * u * (one - v) + tap(x1, y1) * u * v
    return (f + o).astype(dtype)


def flow_pyramids(f0, f1, b0, b1, levels, factors, dtype=np.float64):
    """the four flow families through the level loop, as oracle.flow_pyramids walks it"""
    fam = {k: [np.asarray(x, dtype) for x in v] for k, v in (("f0", f0), ("f1", f1), ("b0", b0), ("b1", b1))}
    out = []
    prev_d = levels[0][2]
    for el, (w, h, d) in enumerate(levels[:-1]):
        ft = factors[el]
        for k in fam:
            fam[k] = [flow_scale(fl, w, h, dtype) for fl in fam[k][:prev_d]]
        if el > 0 and ft > 1:
            for t in range(d):
                if t * ft > prev_d - 1:
                    continue
                if t * ft + 1 < prev_d:
                    for k in ("f0", "f1"):
                        fam[k][t * ft] = flow_concat(fam[k][t * ft], fam[k][t * ft + 1], dtype)
                if t > 0:
                    for k in ("b0", "b1"):
                        fam[k][t * ft] = flow_concat(fam[k][t * ft], fam[k][t * ft - 1], dtype)
            for k in fam:
                fam[k] = [fam[k][min(t * ft, prev_d - 1)].copy() for t in range(d)]
        out.append({k: [a.copy() for a in fam[k][:d]] for k in fam})
        prev_d = d
    return out
