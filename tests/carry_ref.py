"""The float32 numpy statement of what videomorphing_amd/csrc/vm_carry.hip computes (include/vmorph.h): a
point q of the output frame at the from-time carried to its position at other times of the morph.  The chain is the
renderer's (warp_ref.sampling_maps / transit_ref.transition_maps) started from q instead of a pixel centre; after its 20
rounds it holds the halfway point p, the damped V and the damped U, and the position at a to-time g is closed form:
(p + s1(g) V) + s2(g) U with s1 = 2 g - 1, s2 = 4 g - 4 g g.  Under a schedule the rate at p for a to-time t_k is the
chain's own rate tap on the geometry schedule ramped at t_k.  The taps are warp_ref.tap, the rate tap and the ramp
transit_ref's.  tests/test_carry_ref.py pins the statement to those two without a GPU; tests/test_gpu_carry.py holds the
kernels to it bit for bit."""
import numpy as np

import transit_ref as T
import warp_ref as R

f32 = np.float32
HALF, ONE = R.HALF, R.ONE


def _chain(v, u, qx, qy, rate):
    """the 20 rounds from (qx, qy); rate(px, py) is g at p (a constant for the uniform call) -> px, py, lx, ly, V, U"""
    px, py = qx.copy(), qy.copy()
    lx, ly = px, py
    V, U = R.tap(v, px + HALF, py + HALF), R.tap(u, px + HALF, py + HALF)
    g = rate(px, py)
    for _ in range(R.ITERS):
        lx, ly = px, py
        s1 = f32(2) * g - ONE
        s2 = f32(4) * g - f32(4) * g * g
        px = (qx - s1 * V[..., 0]) - s2 * U[..., 0]
        py = (qy - s1 * V[..., 1]) - s2 * U[..., 1]
        V = R.ALPHA * R.tap(v, px + HALF, py + HALF) + (ONE - R.ALPHA) * V
        U = R.ALPHA * R.tap(u, px + HALF, py + HALF) + (ONE - R.ALPHA) * U
        g = rate(px, py)
    return px, py, lx, ly, V, U


def _inside(m, w, h):
    """warp_ref.inside_flags' comparison for points that are no (h, w) grid: that function reads w and h off the shape
    of its maps, which only the dense call's outputs have (tests/test_carry_ref.py holds the two together on the grid)"""
    return (f32(0) <= m[..., 0]) & (m[..., 0] <= f32(w - 1)) & (f32(0) <= m[..., 1]) & (m[..., 1] <= f32(h - 1))


def _carry(v, u, points, rate, rate_to, times):
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    u = np.zeros((h, w, 2), f32) if u is None else np.ascontiguousarray(u, dtype=f32)
    q = np.ascontiguousarray(points, dtype=f32)
    assert q.shape[-1] == 2
    with np.errstate(all="ignore"):
        px, py, lx, ly, V, U = _chain(v, u, q[..., 0], q[..., 1], rate)
        halfway = np.stack([px, py], -1)
        pos0 = np.stack([px - V[..., 0], py - V[..., 1]], -1)
        pos1 = np.stack([px + V[..., 0], py + V[..., 1]], -1)
        resid = np.fmax(np.abs(px - lx), np.abs(py - ly))
        flags = (_inside(pos0, w, h).astype(np.uint8) | (_inside(pos1, w, h).astype(np.uint8) << 1)).astype(np.uint8)
        out = np.empty((len(times),) + q.shape, f32)
        for k, t in enumerate(times):
            g = rate_to(px, py, t)
            s1 = f32(2) * g - ONE
            s2 = f32(4) * g - f32(4) * g * g
            out[k, ..., 0] = (px + s1 * V[..., 0]) + s2 * U[..., 0]
            out[k, ..., 1] = (py + s1 * V[..., 1]) + s2 * U[..., 1]
    assert halfway.dtype == f32 and pos0.dtype == f32 and pos1.dtype == f32 and resid.dtype == f32
    return out, halfway, pos0, pos1, resid, flags


def carry(v, u, points, from_fa, to_fa):
    """(out (nt, ..., 2), halfway, pos0, pos1 (..., 2), resid, flags (...)) of the points (..., 2) of the output frame at
    from_fa, carried to every time of to_fa; v the field, u the path (None: no path, s2 * 0 still added).  No time is
    clamped."""
    geo = f32(from_fa)
    return _carry(v, u, points, lambda px, py: geo, lambda px, py, t: f32(t), [f32(t) for t in np.atleast_1d(to_fa)])


def carry_transition(v, u, sched_geo, points, t_from, t_to, ease):
    """carry under the geometry schedule sched_geo ((h, w, 2) pairs (t0, t1); None: uniform): the chain runs with the
    rates of the plane ramped at t_from, and the rate of a to-time t_k is the same tap at p on the plane ramped at t_k.
    The colour plane plays no part."""
    v = np.ascontiguousarray(v, dtype=f32)
    h, w = v.shape[:2]
    sched = T.uniform_schedule(w, h) if sched_geo is None else sched_geo
    G = T.ramp(sched, t_from, ease)
    return _carry(v, u, points, lambda px, py: T.tapr(G, px + HALF, py + HALF),
                  lambda px, py, t: T.tapr(T.ramp(sched, t, ease), px + HALF, py + HALF), [f32(t) for t in np.atleast_1d(t_to)])


def grid(w, h):
    """the pixel centres of a w x h frame as points: (h, w, 2)"""
    qy, qx = np.mgrid[0:h, 0:w].astype(f32)
    return np.stack([qx, qy], -1)


def gaps(pos1_of_l, pos0_of_r, cons):
    """the distances of constraint_gaps from the carried points, float32: |pos1(l) - r|, |pos0(r) - l|"""
    c = np.asarray(cons, dtype=f32).reshape(-1, 5)[:, :4]
    with np.errstate(all="ignore"):
        d01 = np.hypot(pos1_of_l[:, 0] - c[:, 2], pos1_of_l[:, 1] - c[:, 3])
        d10 = np.hypot(pos0_of_r[:, 0] - c[:, 0], pos0_of_r[:, 1] - c[:, 1])
    assert d01.dtype == f32 and d10.dtype == f32
    return d01, d10


def constraint_gaps(v, u, cons):
    """how well each constraint row (lx, ly, rx, ry, weight) is met, in pixels: (lx, ly) carried from image 0 (time 0)
    gives pos1, compared with (rx, ry); (rx, ry) carried from image 1 (time 1) gives pos0, compared with (lx, ly) ->
    (gap01, gap10, resid01, resid10), one float32 per row each"""
    c = np.asarray(cons, dtype=f32).reshape(-1, 5)
    if not len(c):
        return tuple(np.empty(0, f32) for _ in range(4))
    _, _, _, p1, r01, _ = carry(v, u, c[:, 0:2], 0.0, [1.0])
    _, _, p0, _, r10, _ = carry(v, u, c[:, 2:4], 1.0, [0.0])
    d01, d10 = gaps(p1, p0, c)
    return d01, d10, r01, r10
