"""The error view of DESIGN.md 3.8 stated in numpy: the five float32 planes (np.float32 operations in the stated
order), their totals (float64, one fixed order), the image (the sampling of k_upscale / MatchingThread.cpp:103-136 on a
scalar plane, gain, clamp, heat ramp) and the cases the CPU and GPU tests share.  Test infrastructure: the product never
imports it."""
import math

import numpy as np

F = np.float32
SSIM, TPS, UI, TEMP, ALL = range(5)

# level sizes of the GPU tests: one partial workgroup; width no multiple of 64 and height no multiple of 4; the smoke
# shape; several workgroups per row and a last-arriver fold over many partials (4 x 33 = 132 workgroups, 5 ticket groups)
SHAPES = [(9, 7), (67, 33), (138, 84), (255, 130)]


def constraints(w, h):
    """three point pairs inside any of SHAPES (full-resolution = level coordinates), so that ui_axy > 0 somewhere"""
    return np.asarray([(0.25 * w, 0.30 * h, 0.25 * w + 1.0, 0.30 * h + 0.5, 1.0),
                       (0.70 * w, 0.55 * h, 0.70 * w - 1.5, 0.55 * h + 1.0, 0.5),
                       (0.50 * w, 0.80 * h, 0.50 * w + 0.5, 0.80 * h - 1.0, 1.0)], dtype=np.float32)


def planes(value, v, tps_b, ui_axy, ui_b, inv_wh, P, temp_ref=None, temp_mask=None, factor_d=1.0):
    """(5, h, w) float32: e_ssim, e_tps, e_ui, e_temp, e_all.  P: anything with w_ssim, w_tps, w_ui, w_temp;
    temp_mask is None <=> flag == false."""
    value, v, tps_b, ui_axy, ui_b = (np.asarray(a, dtype=F) for a in (value, v, tps_b, ui_axy, ui_b))
    inv_wh = F(inv_wh)
    w_ssim, w_tps, w_ui, w_temp = F(P.w_ssim), F(P.w_tps), F(P.w_ui), F(P.w_temp)
    e = np.zeros((5,) + value.shape, dtype=F)
    e[SSIM] = (w_ssim * (F(1.0) - value)) * inv_wh
    e[TPS] = w_tps * (F(0.5) * (v[..., 0] * tps_b[..., 0] + v[..., 1] * tps_b[..., 1]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ui = (w_ui * ((ui_b[..., 0] * ui_b[..., 0] + ui_b[..., 1] * ui_b[..., 1]) / (F(4.0) * ui_axy))) * inv_wh
    e[UI] = np.where(ui_axy > 0, ui, F(0.0))
    if temp_mask is not None:
        ref, mask = np.asarray(temp_ref, dtype=F), np.asarray(temp_mask, dtype=F)
        e[TEMP] = (((w_temp * (np.abs(v[..., 0] - ref[..., 0]) + np.abs(v[..., 1] - ref[..., 1]))) * mask) * F(factor_d)) * inv_wh
    e[ALL] = ((e[SSIM] + e[TPS]) + e[UI]) + e[TEMP]
    assert e.dtype == F
    return e


def totals(e):
    """the five sums in float64, each plane folded row-major in sequence"""
    return np.array([np.cumsum(p.astype(np.float64).ravel())[-1] for p in e])


def exact_totals(e):
    return np.array([math.fsum(p.astype(np.float64).ravel().tolist()) for p in e])


def sum_bound(p):
    """what a float64 fold of the n values of plane p, in any order, may differ from their exact sum by: n 2^-53 sum |e|"""
    return p.size * 2.0 ** -53 * float(np.abs(p.astype(np.float64)).sum())


def statement_bound(p):
    """float32 planes against the float64 statement of vmo_energy: at most six float32 roundings per value (factor 8
    covers them), plus the summation bound"""
    return 8 * 2.0 ** -24 * float(np.abs(p.astype(np.float64)).sum()) + sum_bound(p)


def sample(plane, w0, h0):
    """k_upscale's sampling (vm_render.hip; MatchingThread.cpp:103-136) of a scalar plane, NOT rescaled by the ratio"""
    plane = np.asarray(plane, dtype=F)
    h, w = plane.shape
    if (w, h) == (w0, h0):
        return plane.copy()
    fy = ((np.arange(h0, dtype=np.float64) + 0.5) / h0 * h - 0.5).astype(F)
    fx = ((np.arange(w0, dtype=np.float64) + 0.5) / w0 * w - 0.5).astype(F)
    x0, x1, y0, y1 = np.floor(fx), np.ceil(fx), np.floor(fy), np.ceil(fy)
    uu, vv = (fx - x0)[None, :], (fy - y0)[:, None]
    cx = lambda a: np.clip(a.astype(np.int64), 0, w - 1)[None, :]
    cy = lambda a: np.clip(a.astype(np.int64), 0, h - 1)[:, None]
    v00, v01, v10, v11 = plane[cy(y0), cx(x0)], plane[cy(y1), cx(x0)], plane[cy(y0), cx(x1)], plane[cy(y1), cx(x1)]
    one = F(1)
    s = v00 * (one - uu) * (one - vv) + v01 * (one - uu) * vv + v10 * uu * (one - vv) + v11 * uu * vv
    assert s.dtype == F
    return s


def ramp(s, gain):
    """t = clamp(s gain, 0, 1) through the heat ramp to RGB8 (h, w, 3)"""
    t = np.minimum(np.maximum(np.asarray(s, dtype=F) * F(gain), F(0)), F(1))
    r = np.minimum(F(3) * t, F(1))
    g = np.minimum(np.maximum(F(3) * t - F(1), F(0)), F(1))
    b = np.minimum(np.maximum(F(3) * t - F(2), F(0)), F(1))
    rgb = np.stack([r, g, b], axis=-1) * F(255) + F(0.5)
    assert rgb.dtype == F
    return rgb.astype(np.uint8)


def image(plane, w0, h0, gain):
    return ramp(sample(plane, w0, h0), gain)
