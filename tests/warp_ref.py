"""The float32 numpy statement of what videomorphing_amd/csrc/vm_warp.hip computes: the fixed point of the compositor
(kernel_render_halfway_image, render.cu:16-60) with its two sampling positions kept, the move of its last round, the
inside flags, and float layers sampled at those positions.  Every scalar is a float32, every expression stands in the
kernels' order (they are built without contraction), fmaxf / fminf are np.fmax / np.fmin (a NaN loses), and
(px + 0.5) - 0.5 is formed the way the kernels form it.  tests/test_warp_ref.py pins the statement to the renderer's
verified arithmetic without a GPU (its maps, sampled on the extended canvases, give the oracle's bytes);
tests/test_gpu_layers.py holds the kernels to it bit for bit."""
import numpy as np

f32 = np.float32
HALF, ONE = f32(0.5), f32(1)
ITERS = 20              # render.cu:29
ALPHA = f32(0.8)


def tap(img, x, y):
    """tap2 of vm_render.hip on an (h, w, C) float32 image at texture coordinates (x, y) (texel i at i + 0.5):
    clamp-to-edge indices, (1-a)(1-b) t00 + a(1-b) t10 + (1-a)b t01 + ab t11 from left to right, per channel"""
    h, w = img.shape[:2]
    xb, yb = x - HALF, y - HALF
    fi, fj = np.floor(xb), np.floor(yb)
    a, b = xb - fi, yb - fj
    fi = np.fmin(np.fmax(fi, f32(-1)), f32(w))
    fj = np.fmin(np.fmax(fj, f32(-1)), f32(h))
    i0, j0 = fi.astype(np.int64), fj.astype(np.int64)
    i1, j1 = np.clip(i0 + 1, 0, w - 1), np.clip(j0 + 1, 0, h - 1)
    i0, j0 = np.clip(i0, 0, w - 1), np.clip(j0, 0, h - 1)
    w00, w10 = ((ONE - a) * (ONE - b))[..., None], (a * (ONE - b))[..., None]
    w01, w11 = ((ONE - a) * b)[..., None], (a * b)[..., None]
    return ((w00 * img[j0, i0] + w10 * img[j0, i1]) + w01 * img[j1, i0]) + w11 * img[j1, i1]


def sampling_maps(v, u, geo_fa):
    """(map0, map1, resid, flags) of a frame with the field v and the path u ((h, w, 2) float32; u None: the no-path
    form -- a zero path stays zero through the rounds, and s2 * 0 is still subtracted, as the kernels do)"""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    geo = f32(geo_fa)
    with np.errstate(all="ignore"):
        s1 = f32(2) * geo - ONE
        s2 = f32(4) * geo - f32(4) * geo * geo
        qy, qx = np.mgrid[0:h, 0:w].astype(f32)
        px, py = qx.copy(), qy.copy()
        V, U = tap(v, px + HALF, py + HALF), tap(u, px + HALF, py + HALF)
        for _ in range(ITERS):
            lx, ly = px, py
            px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
            py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
            V = ALPHA * tap(v, px + HALF, py + HALF) + (ONE - ALPHA) * V
            U = ALPHA * tap(u, px + HALF, py + HALF) + (ONE - ALPHA) * U
        map0 = np.stack([px - V[..., 0], py - V[..., 1]], -1)
        map1 = np.stack([px + V[..., 0], py + V[..., 1]], -1)
        resid = np.fmax(np.abs(px - lx), np.abs(py - ly))
    assert map0.dtype == f32 and map1.dtype == f32 and resid.dtype == f32
    return map0, map1, resid, inside_flags(map0, map1)


def inside_flags(map0, map1):
    """bit 0: 0 <= map0.x <= w - 1 and 0 <= map0.y <= h - 1; bit 1: the same for map1 (a NaN fails every comparison)"""
    h, w = map0.shape[:2]
    with np.errstate(invalid="ignore"):
        def inside(m):
            return (f32(0) <= m[..., 0]) & (m[..., 0] <= f32(w - 1)) & (f32(0) <= m[..., 1]) & (m[..., 1] <= f32(h - 1))
        return (inside(map0).astype(np.uint8) | (inside(map1).astype(np.uint8) << 1)).astype(np.uint8)


def blend(c0, c1, color_fa, color_from):
    """color_from 0: c0, 2: c1, 1: c0 * (1 - color_fa) + c1 * color_fa in float32"""
    col = f32(color_fa)
    if color_from == 0:
        return c0
    if color_from == 2:
        return c1
    with np.errstate(all="ignore"):
        return c0 * (ONE - col) + c1 * col


def render_layers(layer0, layer1, map0, map1, color_fa, color_from):
    """two (h, w) or (h, w, C) float32 layers sampled at (map + 0.5) on the layer itself (the edge texel repeats) and
    blended: float32 of the layers' shape"""
    l0, l1 = np.asarray(layer0, dtype=f32), np.asarray(layer1, dtype=f32)
    shape = l0.shape
    if l0.ndim == 2:
        l0, l1 = l0[..., None], l1[..., None]
    with np.errstate(all="ignore"):
        c0 = tap(l0, map0[..., 0] + HALF, map0[..., 1] + HALF)
        c1 = tap(l1, map1[..., 0] + HALF, map1[..., 1] + HALF)
    out = blend(c0, c1, color_fa, color_from)
    assert out.dtype == f32
    return out.reshape(shape)


def render_bytes(ext0, ext1, ex, map0, map1, color_fa, color_from):
    """the renderer's tail on the maps: the extended RGBA8 canvases sampled at (map + ex) + 0.5, blended, + 0.5 in
    double, truncated (render.cu:39-57) -> (h, w, 3) uint8"""
    exf = f32(ex)
    with np.errstate(all="ignore"):
        c0 = tap(ext0[..., :3].astype(f32), (map0[..., 0] + exf) + HALF, (map0[..., 1] + exf) + HALF)
        c1 = tap(ext1[..., :3].astype(f32), (map1[..., 0] + exf) + HALF, (map1[..., 1] + exf) + HALF)
        return (blend(c0, c1, color_fa, color_from).astype(np.float64) + 0.5).astype(np.uint8)


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
