"""The numpy statement of transition control (tests/transit_ref.py) pinned to the statement of the uniform chain
(tests/warp_ref.py), without a GPU: under the schedule (0, 1) with the linear ease it IS the uniform chain, bit for bit;
two half frames scheduled one after the other equal the two uniform extremes away from their seam; the ramp's corner
cases are what include/vmorph.h says; a rate tap of a constant plane is that constant to the bit."""

import numpy as np
import pytest

import chain_ref
import transit_ref as T
from render_cases import field as _field
import warp_ref as R

f32 = np.float32


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("w,h", [(70, 37), (203, 77), (5, 3)])
@pytest.mark.parametrize("kind", ["smooth", "rough", "large", "shear", "outside"])
@pytest.mark.parametrize("with_path", [False, True])
def test_uniform_schedule_is_the_uniform_chain(w, h, kind, with_path):
    """schedule (0, 1), linear ease: G is exactly t, and maps, resid and flags are warp_ref.sampling_maps(v, u, t)'s bits"""
    v, u = _field(w, h, kind, with_path)
    for t in (0.0, 0.2, 0.35, 0.5, 0.8, 1.0):
        assert np.all(T.ramp(T.uniform_schedule(w, h), t, T.EASE_LINEAR).view(np.uint32) == f32(t).view(np.uint32))
        got = T.transition_maps(v, u, None, None, t, T.EASE_LINEAR)
        want = R.sampling_maps(v, u, t)
        for n, g, r in zip(("map0", "map1", "resid", "flags"), got, want):
            assert g.dtype == r.dtype and np.array_equal(_bits(g), _bits(r)), (n, t)
        assert np.all(got[4].view(np.uint32) == f32(t).view(np.uint32))


@pytest.mark.parametrize("w,h,compared", [(203, 77, 193), (138, 84, 130)])
def test_two_halves_equal_the_uniform_extremes_away_from_the_seam(w, h, compared):
    v, u = _field(w, h, "smooth", True)
    left, right = T.two_halves_columns(v, w)
    assert len(left) + len(right) == compared and 4 * compared >= 3 * w
    band = np.arange(left[-1] + 1, right[0])
    one, zero = R.sampling_maps(v, u, 1.0), R.sampling_maps(v, u, 0.0)
    for ease in (T.EASE_LINEAR, T.EASE_SMOOTH):
        got = T.transition_maps(v, u, T.two_halves(w, h), None, 0.5, ease)
        for n, g, a, b in zip(("map0", "map1", "resid", "flags"), got, one, zero):
            assert np.array_equal(_bits(g[:, left]), _bits(a[:, left])), (n, ease, "left")
            assert np.array_equal(_bits(g[:, right]), _bits(b[:, right])), (n, ease, "right")
        for a in (one, zero):
            assert not np.array_equal(got[0][:, band], a[0][:, band])


def test_ramp_corner_cases():
    def ramp1(t0, t1, t, ease=T.EASE_LINEAR):
        return T.ramp(np.array([[[t0, t1]]], f32), t, ease)[0, 0]

    # t1 < t0 and t1 == t0: a step at t0, which t == t0 has taken
    for t0, t1 in ((0.5, 0.2), (0.5, 0.5)):
        for ease in (T.EASE_LINEAR, T.EASE_SMOOTH):
            assert ramp1(t0, t1, 0.49, ease) == 0 and ramp1(t0, t1, 0.5, ease) == 1 and ramp1(t0, t1, 7.0, ease) == 1
    # t outside [0, 1] is not clamped, the ramp is
    assert ramp1(-1.0, 3.0, 0.0) == f32(0.25) and ramp1(-1.0, 3.0, -2.0) == 0 and ramp1(-1.0, 3.0, 4.0) == 1
    assert ramp1(0.0, 1.0, -0.5) == 0 and ramp1(0.0, 1.0, 1.5) == 1
    # float32 in the stated order: (t - t0) / d, correctly rounded
    assert ramp1(0.1, 0.7, 0.3).view(np.uint32) == ((f32(0.3) - f32(0.1)) / (f32(0.7) - f32(0.1))).view(np.uint32)
    # the smooth ease: exactly 0 and 1 at the ends, (s s)(3 - 2 s) between
    assert ramp1(0.0, 1.0, 0.0, T.EASE_SMOOTH).view(np.uint32) == f32(0).view(np.uint32)
    assert ramp1(0.0, 1.0, 1.0, T.EASE_SMOOTH).view(np.uint32) == f32(1).view(np.uint32)
    s = f32(0.3)
    assert ramp1(0.0, 1.0, 0.3, T.EASE_SMOOTH).view(np.uint32) == ((s * s) * (f32(3) - f32(2) * s)).view(np.uint32)
    assert ramp1(0.0, 1.0, 0.5, T.EASE_SMOOTH) == f32(0.5)
    # a NaN start loses every comparison
    assert ramp1(np.nan, 1.0, 0.5) == 0
    with pytest.raises(AssertionError):
        T.ramp(T.uniform_schedule(2, 2), 0.5, 2)


def test_rate_tap_of_a_constant_plane_is_the_constant():
    """the lerp form returns a constant plane's value exactly; the four-weight form of chain_ref.tap does not"""
    rng = np.random.RandomState(7)
    w, h = 37, 23
    x = (rng.rand(4000) * (w + 8) - 4).astype(f32)
    y = (rng.rand(4000) * (h + 8) - 4).astype(f32)
    four_weights_differ = False
    for c in (0.2, 0.35, 1.0 / 3.0, 0.8, 1.0, 0.0):
        plane = np.full((h, w), c, f32)
        assert np.all(chain_ref.tapr(plane, x, y).view(np.uint32) == f32(c).view(np.uint32)), c
        four_weights_differ |= bool(np.any(chain_ref.tap(plane[..., None], x, y)[..., 0] != f32(c)))
    assert four_weights_differ
    # and between two texels it is the lerp
    plane = np.zeros((2, 2), f32)
    plane[:, 1] = 1
    assert chain_ref.tapr(plane, np.array([1.25], f32), np.array([1.0], f32))[0] == f32(0.75)


def test_schedule_builders():
    """videomorphing_amd/transition.py: starts spread over [0, lead] along the wipe's direction, from the radial centre
    outwards and from a matte's foreground to its background; one duration for every texel"""
    from videomorphing_amd import transition
    w, h = 23, 11
    for s in (transition.wipe(w, h, (1.0, 0.0), lead=0.6, duration=0.4), transition.radial(w, h, (3, 4), lead=0.6, duration=0.4)):
        assert s.shape == (h, w, 2) and s.dtype == f32
        assert s[..., 0].min() == 0 and s[..., 0].max() == f32(0.6) and np.allclose(s[..., 1] - s[..., 0], 0.4, atol=1e-6)
    s = transition.wipe(w, h, (1.0, 0.0), lead=0.6, duration=0.4)
    assert np.all(np.diff(s[..., 0], axis=1) > 0) and np.all(s[..., 0] == s[:1, :, 0])
    assert np.all(transition.wipe(w, h, (-1.0, 0.0))[..., 0] == s[:, ::-1, 0])
    r = transition.radial(w, h, (3, 4))
    assert r[4, 3, 0] == 0 and r[..., 0].argmax() == np.ravel_multi_index((h - 1, w - 1), (h, w))
    matte = np.zeros((h, w))
    matte[:, :5] = 1.0
    matte[:, 5] = 0.5
    m = transition.from_matte(matte, lead=0.4)
    assert np.all(m[:, :5, 0] == 0) and np.all(m[:, 5, 0] == f32(0.2)) and np.all(m[:, 6:, 0] == f32(0.4))
    assert np.allclose(m[..., 1] - m[..., 0], 0.6, atol=1e-6)
    assert np.array_equal(transition.uniform(w, h), T.uniform_schedule(w, h))
    # the foreground is ahead of the background at every time in between
    g = T.ramp(m, 0.5, T.EASE_SMOOTH)
    assert g[:, :5].min() > g[:, 6:].max() > 0
