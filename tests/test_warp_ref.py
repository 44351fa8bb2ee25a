"""The numpy statement of the warp kernels (tests/warp_ref.py) against the renderer's verified arithmetic and against
its own definitions.  CPU only: the oracle is the C statement of render.cu:16-60 the GPU renderer is held to."""
import numpy as np
import pytest

import warp_ref
from videomorphing_amd import morph, synth

f32 = np.float32
SIZES = [(203, 77, 9), (33, 7, 0), (5, 3, 2)]


def _grid(w, h):
    yy, xx = np.mgrid[0:h, 0:w].astype(f32)
    return np.stack([xx, yy], -1)


@pytest.mark.parametrize("w,h,ex", SIZES)
def test_statement_maps_give_the_oracles_bytes(oracle, w, h, ex):
    """the maps of the statement, sampled on the extended canvases at (map + ex) + 0.5 with the renderer's double + 0.5
    and truncation, are oracle.render_halfway's bytes: 3 sizes x (smooth, rough, outside) x (no path, path) x geo_fa
    (0, 0.35, 1) = 54 cases, zero differing bytes"""
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    rng = np.random.RandomState(41)
    ncases = 0
    for kind in ("smooth", "rough", "outside"):
        v = warp_ref.field(kind, w, h, rng)
        for with_path in (False, True):
            u = warp_ref.path(w, h, rng) if with_path else None
            uo = u if with_path else np.zeros((h, w, 2), f32)
            for geo in (0.0, 0.35, 1.0):
                m0, m1, _, _ = warp_ref.sampling_maps(v, u, geo)
                out = warp_ref.render_bytes(e0, e1, ex, m0, m1, 0.3, 1)
                ref = oracle.render_halfway(w, h, ex, 0.3, geo, 1, e0.astype(f32), e1.astype(f32), v, uo)
                assert np.array_equal(out, ref), (kind, with_path, geo, int((out != ref).sum()))
                ncases += 1
    assert ncases == 18


@pytest.mark.parametrize("w,h,ex", SIZES)
@pytest.mark.parametrize("with_path", [False, True])
def test_identity(w, h, ex, with_path):
    """v = u = 0: the maps are the pixel grid exactly, nothing moves, everything is inside, layers come back bit for bit"""
    v = np.zeros((h, w, 2), f32)
    u = np.zeros((h, w, 2), f32) if with_path else None
    rng = np.random.RandomState(5)
    l0, l1 = rng.randn(h, w, 3).astype(f32) * f32(100), rng.randn(h, w, 3).astype(f32)
    for geo in (0.0, 0.35, 1.0):
        m0, m1, resid, flags = warp_ref.sampling_maps(v, u, geo)
        assert np.array_equal(m0, _grid(w, h)) and np.array_equal(m1, _grid(w, h))
        assert np.all(resid == 0) and np.all(flags == 3)
        assert np.array_equal(warp_ref.render_layers(l0, l1, m0, m1, 0.3, 0).view(np.uint32), l0.view(np.uint32))
        assert np.array_equal(warp_ref.render_layers(l0, l1, m0, m1, 0.3, 2).view(np.uint32), l1.view(np.uint32))
        assert np.array_equal(warp_ref.render_layers(l0[..., 0], l1[..., 0], m0, m1, 0.3, 0), l0[..., 0])


@pytest.mark.parametrize("w,h,ex", SIZES)
def test_forward_correspondence(w, h, ex):
    """at geo_fa = 0 the fixed point solves p = q + v(p): image 0 is sampled at p - v(p) = q, the output pixel itself,
    and map1 = q + 2 v(p) is the forward map image 0 -> image 1.  On the smooth field (amplitude 0.01 w over one period:
    |grad v| < 0.07, so a round multiplies the error by less than 0.2 + 0.8 * 0.07 < 0.26 and 20 rounds leave nothing of
    the first guess's few pixels; float32 rounding of coordinates below 256 is 3e-5) |map0 - grid| <= 1e-3 px: a
    condition, not a measurement."""
    v = warp_ref.field("smooth", w, h, None)
    m0, m1, resid, flags = warp_ref.sampling_maps(v, None, 0.0)
    assert np.abs(m0 - _grid(w, h)).max() <= 1e-3
    assert resid.max() <= 1e-3
    # ... and the backward map at geo_fa = 1
    m0, m1, _, _ = warp_ref.sampling_maps(v, None, 1.0)
    assert np.abs(m1 - _grid(w, h)).max() <= 1e-3


def test_flags_follow_their_definition():
    """on the field whose taps leave the image on every side: the flags are the definition, pixel by pixel, and both
    values of both bits occur (over the geo_fa: at geo_fa = 0 every sample of image 1 is outside)"""
    w, h = 203, 77
    v = warp_ref.field("outside", w, h, None)
    seen = {0: set(), 1: set()}
    for geo in (0.0, 0.35, 0.5, 1.0):
        m0, m1, _, flags = warp_ref.sampling_maps(v, None, geo)
        for bit, m in ((0, m0), (1, m1)):
            got = (flags >> bit) & 1
            want = np.zeros((h, w), np.uint8)
            for y in range(h):
                for x in range(w):
                    want[y, x] = 0.0 <= float(m[y, x, 0]) <= w - 1 and 0.0 <= float(m[y, x, 1]) <= h - 1
            assert np.array_equal(got, want)
            seen[bit] |= set(np.unique(got).tolist())
    assert seen == {0: {0, 1}, 1: {0, 1}}
    m = np.full((2, 2, 2), np.nan, f32)
    assert np.all(warp_ref.inside_flags(m, m) == 0)
