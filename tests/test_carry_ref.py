"""tests/carry_ref.py -- the statement of the carry calls (vm_frame_carry_points, vm_frame_motion_maps and their forms
under a schedule) -- pinned without a GPU to arithmetic the project has already verified: started from the
pixel grid with the to-times {0, 1} it is warp_ref.sampling_maps (transit_ref.transition_maps under a schedule), a zero
or constant field carries a point where arithmetic says, and a point carried there and back returns.

Shapes are those of the warp tests: 203x77 is no multiple of the 32x16 tile, 33x7 narrower than the LDS window, 5x3
smaller than the window's margin (every clamp), 138x84 the smoke shape; the kinds are tests/render_cases.py's."""
import os

import numpy as np
import pytest

import carry_ref
import transit_ref
import warp_ref
from render_cases import field as _field, same_bits
from videomorphing_amd import capi, transition

f32 = np.float32
SHAPES = [(203, 77), (33, 7), (5, 3), (138, 84)]
KINDS = ["smooth", "rough", "large", "shear", "outside", "nan"]
FROMS = (0.0, 0.2, 0.5, 1.0)
NEW_SYMBOLS = ("vm_frame_carry_points", "vm_frame_carry_points_transition", "vm_frame_motion_maps", "vm_frame_motion_maps_dev",
               "vm_frame_transition_motion_maps", "vm_frame_transition_motion_maps_dev")


def same_numbers(got, want):
    """as numbers (+0 == -0), a NaN for a NaN"""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


def test_the_entry_points_are_declared():
    assert set(NEW_SYMBOLS) <= set(capi.SYMBOLS)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vmorph.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_grid_to_both_images_is_the_sampling_maps(w, h, kind):
    """from the pixel grid with the to-times {0, 1}: out is map0 / map1 of warp_ref.sampling_maps, pos0 / pos1 / resid /
    flags its four outputs"""
    for with_path in (False, True):
        v, u = _field(w, h, kind, with_path)
        for fa in FROMS:
            out, halfway, pos0, pos1, resid, flags = carry_ref.carry(v, u, carry_ref.grid(w, h), fa, [0.0, 1.0])
            m0, m1, r, fl = warp_ref.sampling_maps(v, u, fa)
            case = (with_path, fa)
            assert same_numbers(out[0], m0) and same_numbers(out[1], m1), case
            assert same_numbers(pos0, m0) and same_numbers(pos1, m1), case
            assert same_numbers(resid, r) and same_numbers(flags, fl), case
            assert out.shape == (2, h, w, 2) and halfway.shape == (h, w, 2)


def _schedule(w, h, name):
    if name == "wipe":
        return transition.wipe(w, h, (1.0, 0.3), lead=0.6, duration=0.4)
    return transition.radial(w, h, (0.3 * w, 0.6 * h), lead=0.5, duration=0.5)


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["wipe", "radial"])
def test_grid_under_a_schedule_is_the_transition_maps(w, h, kind, name):
    """the same -- all shapes, all kinds, with and without a path, from 0, 0.2, 0.5, 1, both eases -- under a wipe and a
    radial schedule, against transit_ref.transition_maps.  The rate of a to-time is the
    ramp of the schedule at that time: before every texel has started it is 0 (image 0), after every texel has arrived 1
    (image 1) -- the two to-times that have a verified counterpart."""
    sched = _schedule(w, h, name)
    before, after = float(sched[..., 0].min()) - 0.25, float(sched[..., 1].max()) + 0.25
    for with_path in (False, True):
        v, u = _field(w, h, kind, with_path)
        for t, ease in ((t, ease) for t in FROMS for ease in (transit_ref.EASE_LINEAR, transit_ref.EASE_SMOOTH)):
            out, _, pos0, pos1, resid, flags = carry_ref.carry_transition(v, u, sched, carry_ref.grid(w, h), t, [before, after], ease)
            m0, m1, r, fl, _ = transit_ref.transition_maps(v, u, sched, None, t, ease)
            case = (with_path, t, ease)
            assert same_numbers(out[0], m0) and same_numbers(out[1], m1), case
            assert same_numbers(pos0, m0) and same_numbers(pos1, m1), case
            assert same_numbers(resid, r) and same_numbers(flags, fl), case


@pytest.mark.parametrize("w,h", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_uniform_schedule_gives_the_uniform_bits(w, h, kind):
    """the schedule (0, 1), linear, all times in [0, 1]: every output has the bits of the uniform call"""
    rng = np.random.RandomState(7)
    pts = (rng.rand(97, 2) * (w + 4, h + 4) - 2).astype(f32)
    times = [0.0, 0.25, 0.6, 1.0]
    for with_path in (False, True):
        v, u = _field(w, h, kind, with_path)
        for fa in FROMS:
            uni = carry_ref.carry(v, u, pts, fa, times)
            for sched in (None, transition.uniform(w, h)):
                got = carry_ref.carry_transition(v, u, sched, pts, fa, times, transit_ref.EASE_LINEAR)
                assert all(same_bits(a, b) for a, b in zip(got, uni)), (with_path, fa)


def test_zero_field_returns_the_start_points_bit_for_bit():
    w, h = 33, 7
    rng = np.random.RandomState(3)
    pts = np.concatenate([(rng.rand(64, 2) * (w - 1, h - 1)).astype(f32), f32([[0, 0], [w - 1, h - 1], [1e3, 2e-3], [1e30, 5.5]])])
    v = np.zeros((h, w, 2), f32)
    for u in (None, v):
        out, halfway, pos0, pos1, resid, _ = carry_ref.carry(v, u, pts, 0.3, [0.0, 0.3, 1.0, -0.5, 1.5])
        for k in range(5):
            assert same_bits(out[k], pts), k
        assert same_bits(halfway, pts) and same_bits(pos0, pts) and same_bits(pos1, pts) and not resid.any()


def test_constant_dyadic_field_is_exact():
    """v = (3.5, -2.25) everywhere, no path: a point moves by exactly 2 (to - from) v; the gaps of (10, 5) -> (17, 0.5)
    are exactly 0, and exactly 1 with rx moved by 1"""
    w, h = 33, 17
    v = np.empty((h, w, 2), f32)
    v[...] = (3.5, -2.25)
    pts = f32([[10, 5], [12.5, 7.25], [0, 16], [20.125, 3]])
    for fa, to in ((0.0, 1.0), (0.25, 0.75), (1.0, 0.0), (0.5, 0.5), (0.5, -0.5)):
        out = carry_ref.carry(v, None, pts, fa, [to])[0][0]
        want = pts + f32(2 * (to - fa)) * f32([3.5, -2.25])
        assert same_bits(out, want), (fa, to)
    g01, g10, r01, r10 = carry_ref.constraint_gaps(v, None, [(10, 5, 17, 0.5, 1.0), (10, 5, 18, 0.5, 1.0)])
    assert g01.tolist() == [0.0, 1.0] and g10.tolist() == [0.0, 1.0]
    assert r01.tolist() == [0.0, 0.0] and r10.tolist() == [0.0, 0.0]


def _smooth_path(w, h):
    """a path of the test's own, as smooth as the field (warp_ref.path is white noise and folds)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    return np.stack([1.5 * np.sin(x / 23.0 + 0.4) * np.cos(y / 19.0), 1.2 * np.cos(x / 29.0) * np.sin(y / 17.0 + 1.1)], -1).astype(f32)


ROUND_TRIP_BOUND = 1e-4     # px (x3 over the 3.1e-5 px measured for the statement without a path)


@pytest.mark.parametrize("kind", ["smooth", "large"])
@pytest.mark.parametrize("with_path", [False, True])
def test_round_trip_returns_the_start_points(kind, with_path):
    """carried from s to t and from there back to s, a point returns: within 1e-4 px among the points whose resids on
    both legs are below 1e-3, which are at least 95 % of them.  Holds where the field is invertible: the smooth and the
    large kind, without a path and with a smooth one; 257 random in-domain points.  Measured for this statement with
    these points, at worst over the pairs: 3.05e-5 px (smooth) and 4.58e-5 px (large; three ulps of a coordinate near
    200), all 257 points settled, and with the smooth path the same figures, not higher: the bound of 1e-4 px stands
    for both."""
    w, h = 203, 77
    v, _ = _field(w, h, kind, False)
    u = _smooth_path(w, h) if with_path else None
    rng = np.random.RandomState(11)
    pts = (rng.rand(257, 2) * (w - 1, h - 1)).astype(f32)
    for s, t in ((0.0, 1.0), (0.0, 0.5), (0.3, 0.8), (1.0, 0.0)):
        there, _, _, _, r1, _ = carry_ref.carry(v, u, pts, s, [t])
        back, _, _, _, r2, _ = carry_ref.carry(v, u, there[0], t, [s])
        settled = (r1 < 1e-3) & (r2 < 1e-3)
        worst = float(np.abs(back[0] - pts)[settled].max())
        print("round trip %s path=%d %g -> %g: %d of 257 settled, worst %.3g px" % (kind, with_path, s, t, settled.sum(), worst))
        assert settled.sum() >= 0.95 * len(pts), (s, t, int(settled.sum()))
        assert worst <= ROUND_TRIP_BOUND, (s, t, worst)
