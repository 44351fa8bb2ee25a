"""The numpy statement of what videomorphing_amd/csrc/vm_layer_ext.hip and vm_frame_extend_layers compute: the Poisson
boundary extension (CPoissonExt::prepare + poissonExtend, PoissonExt.cpp:49-362) of a frame's float layers.

    canvas     (ch, cw, C), cw = w + 2 ex, ch = h + 2 ex: the tight layer at (ex, ex), zeros elsewhere; valid = 1 on it
    type map   2 outside the image, 1 on the image's outermost ring, 0 inside (geometric: a layer has no alpha)
    fill       every type-2 cell follows the halfway field -- q = the cell's image coordinates, v = bil_v(q), twenty rounds
               p = q + sign v, v = 0.8f bil_v(p) + (1 - 0.8f) v, then q' = p + sign v -- and takes the OTHER side's tight
               layer at q' bilinearly (floor / ceil, clamps) if q' lies in [0, w) x [0, h), else it is a hole (valid = 0).
               float32, every expression in the kernel's order (it is built without contraction)
    system     unknowns: the cells of type > 0.  diag = [type == 1] + #(4-neighbours of type > 0),  (A x)_i = diag x_i -
               sum of x over those neighbours;  b_i = [type == 1] value_i + g(i, up) + g(i, left) - g(right, i) - g(down, i),
               g(a, b) = value_a - value_b where both are type 2 and valid, else 0
    solution   A x = b per channel (float64 here: conjugate gradients to 1e-12, or dense); every type > 0 cell takes it

and the render tail on extended layers: the tail of tests/chain_ref.py on the (ch, cw, C) canvas at (map + ex) + 0.5.
tests/test_layer_ext_ref.py pins the statement without a GPU, tests/test_gpu_layer_ext.py holds the kernels to it."""
import numpy as np

import chain_ref as C

f32 = np.float32
ONE = f32(1)
AL = f32(0.8)
ROUNDS = 20


def type_map(w, h, ex):
    """(ch, cw) uint8"""
    t = np.full((h + 2 * ex, w + 2 * ex), 2, np.uint8)
    if ex == 0:
        return np.zeros((h, w), np.uint8)
    t[ex:ex + h, ex:ex + w] = 1
    if w > 2 and h > 2:
        t[ex + 1:ex + h - 1, ex + 1:ex + w - 1] = 0
    return t


def canvas(tight, ex):
    """((ch, cw, C) float32, valid (ch, cw) uint8) of a tight (h, w, C) layer"""
    h, w, c = tight.shape
    out = np.zeros((h + 2 * ex, w + 2 * ex, c), f32)
    out[ex:ex + h, ex:ex + w] = tight
    valid = np.zeros(out.shape[:2], np.uint8)
    valid[ex:ex + h, ex:ex + w] = 1
    return out, valid


def _corners(px, py, w, h):
    """floor / ceil indices, clamped, and the weights a, b of BilineaGetColor_clamp (PoissonExt.cpp:367-397)"""
    fx, fy = np.floor(px), np.floor(py)
    a, b = px - fx, py - fy
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    x1, y1 = np.ceil(px).astype(np.int64), np.ceil(py).astype(np.int64)
    cl = lambda i, n: np.clip(i, 0, n - 1)
    return cl(x0, w), cl(x1, w), cl(y0, h), cl(y1, h), a.astype(f32), b.astype(f32)


def bil(img, px, py):
    """img (h, w, K) float32 at (px, py): v00 (1-a)(1-b) + v01 (1-a) b + v10 a (1-b) + v11 a b from left to right, v01 the
    texel below, v10 the texel to the right"""
    h, w = img.shape[:2]
    cx0, cx1, cy0, cy1, a, b = _corners(px, py, w, h)
    a, b = a[..., None], b[..., None]
    v00, v01, v10, v11 = img[cy0, cx0], img[cy1, cx0], img[cy0, cx1], img[cy1, cx1]
    r = v00 * (ONE - a) * (ONE - b) + v01 * (ONE - a) * b + v10 * a * (ONE - b) + v11 * a * b
    assert r.dtype == f32
    return r


def landing(v, ex, sign):
    """(qx, qy) float32 (ch, cw): where every canvas cell's chain lands in the other image (read at the type-2 cells)"""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    sg = f32(sign)
    yy, xx = np.mgrid[0:h + 2 * ex, 0:w + 2 * ex]
    qx, qy = (xx - ex).astype(f32), (yy - ex).astype(f32)
    with np.errstate(all="ignore"):
        px, py = qx, qy
        V = bil(v, px, py)
        for _ in range(ROUNDS):
            px = qx + V[..., 0] * sg
            py = qy + V[..., 1] * sg
            T = bil(v, px, py)
            V = AL * T + (ONE - AL) * V
        lx = px + V[..., 0] * sg
        ly = py + V[..., 1] * sg
    assert lx.dtype == f32 and ly.dtype == f32
    return lx, ly


def prepare(own, other, v, ex, side):
    """(filled (ch, cw, C) float32, valid, type) of side 1 or 2: own / other are the tight (h, w, C) layers of that side
    and of the other one"""
    own, other = np.asarray(own, dtype=f32), np.asarray(other, dtype=f32)
    h, w, _ = own.shape
    typ = type_map(w, h, ex)
    filled, valid = canvas(own, ex)
    lx, ly = landing(v, ex, 1 if side == 1 else -1)
    with np.errstate(all="ignore"):
        inside = (lx >= 0) & (ly >= 0) & (lx < w) & (ly < h)
        val = bil(other, np.where(inside, lx, f32(0)), np.where(inside, ly, f32(0)))
    out = typ == 2
    filled[out & inside] = val[out & inside]
    valid[out & inside] = 1
    return filled, valid, typ


def _shift(a, dy, dx, fill=0):
    """s[y, x] = a[y + dy, x + dx], `fill` where that is off the canvas"""
    s = np.full_like(a, fill)
    h, w = a.shape[:2]
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    s[yd, xd] = a[ys, xs]
    return s


def rhs(filled, valid, typ, dtype):
    """(ch, cw, C) in `dtype`, k_setup's order: the ring's own value, + g(i, up), + g(i, left), - g(right, i), - g(down, i)"""
    val = filled.astype(dtype)
    live = (typ == 2) & (valid != 0)                 # a cell a gradient may use
    zero = dtype(0)

    def g(dy, dx, outward):
        """g(i, nbr) (outward False) or g(nbr, i) (True) for the neighbour at (dy, dx)"""
        both = (live & _shift(live, dy, dx, False))[..., None]
        nb = _shift(val, dy, dx)
        with np.errstate(all="ignore"):
            return np.where(both, (nb - val) if outward else (val - nb), zero)

    with np.errstate(all="ignore"):
        b = np.where((typ == 1)[..., None], zero + val, zero)
        unk = (typ > 0)[..., None]
        for dy, dx, outward in ((-1, 0, False), (0, -1, False), (0, 1, True), (1, 0, True)):
            has = unk & (_shift(typ, dy, dx, 0) > 0)[..., None]
            t = g(dy, dx, outward)
            b = np.where(has, (b - t) if outward else (b + t), b)
    assert b.dtype == dtype
    return b


class Operator(object):
    """the system matrix of a type map, matrix-free (float64): x, b are (ch, cw) or (ch, cw, K); rows of cells that are
    no unknowns are zero"""

    def __init__(self, typ):
        self.unk = typ > 0
        self.nb = [(dy, dx, self.unk & _shift(self.unk, dy, dx, False)) for dy, dx in ((-1, 0), (0, -1), (0, 1), (1, 0))]
        self.diag = (typ == 1).astype(np.float64) + sum(m.astype(np.float64) for _, _, m in self.nb)

    def apply(self, x):
        ex = (lambda m: m[..., None]) if x.ndim == 3 else (lambda m: m)
        y = ex(self.diag) * x
        for dy, dx, m in self.nb:
            y = y - np.where(ex(m), _shift(x, dy, dx), 0.0)
        return np.where(ex(self.unk), y, 0.0)

    def dense(self):
        """(n, n) float64 over the unknowns in row-major order, and their flat indices"""
        idx = np.flatnonzero(self.unk)
        pos = -np.ones(self.unk.size, np.int64)
        pos[idx] = np.arange(idx.size)
        A = np.zeros((idx.size, idx.size))
        A[np.arange(idx.size), np.arange(idx.size)] = self.diag.ravel()[idx]
        cw = self.unk.shape[1]
        for dy, dx, m in self.nb:
            rows = np.flatnonzero(m)
            A[pos[rows], pos[rows + dy * cw + dx]] -= 1.0
        return A, idx


def solve(typ, b, tol=1e-12, max_it=100000):
    """x with A x = b per channel (float64), Jacobi-preconditioned conjugate gradients to a relative residual of `tol` in
    every channel; zero off the unknowns and for a channel whose right-hand side is zero"""
    A = Operator(typ)
    b = np.where(A.unk[..., None], b.astype(np.float64), 0.0)
    x = np.zeros_like(b)
    dinv = np.where(A.unk, 1.0 / np.maximum(A.diag, 1.0), 0.0)[..., None]
    dot = lambda p, q: (p * q).sum((0, 1))
    bb = dot(b, b)
    live = bb > 0
    if not live.any():
        return x
    r = b.copy()
    z = dinv * r
    p = z.copy()
    rz = dot(r, z)
    for _ in range(max_it):
        q = A.apply(p)
        pq = dot(p, q)
        al = np.where(live & (pq > 0), rz / np.where(pq > 0, pq, 1.0), 0.0)
        x = x + al * p
        r = r - al * q
        if (np.sqrt(dot(r, r)[live] / bb[live]) <= tol).all():
            return x
        z = dinv * r
        rz1 = dot(r, z)
        p = z + np.where(rz > 0, rz1 / np.where(rz > 0, rz, 1.0), 0.0) * p
        rz = rz1
    raise AssertionError("layer_ext_ref.solve: no convergence")


def extend(own, other, v, ex, side):
    """the extended layer of one side, float64 (ch, cw, C): the solution on every type > 0 cell, the uploaded value inside;
    and its type map"""
    filled, valid, typ = prepare(own, other, v, ex, side)
    x = solve(typ, rhs(filled, valid, typ, np.float64))
    return np.where((typ > 0)[..., None], x, filled.astype(np.float64)), typ


def render_layers(ext0, ext1, ex, map0, map1, color_fa, color_from):
    """the render tail on extended layers (vm_render_layers on an extended frame): chain_ref.tap on the (ch, cw, C)
    canvases at (map + ex) + 0.5 -- the renderer's own + ex + 0.5f --, blended.  float32 of the maps' grid x C"""
    return C.blended(ext0, ext1, map0, map1, color_fa, color_from, ex)


def layers_on_maps(ext0, ext1, ex, maps, color_fa, color_from):
    """the sample loops' tail on extended layers (the shutter and viewport families): the plates of every (map0, map1) of
    `maps`, blended, summed in float32 in order from +0 and divided by (float)N -- chain_ref's mean"""
    return C.sampled_mean(ext0, ext1, maps, color_fa, color_from, ex)
