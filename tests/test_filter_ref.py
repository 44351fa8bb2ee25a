"""tests/filter_ref.py, the numpy statement of the filtered viewport calls (videomorphing_amd/csrc/vm_filter.hip), pinned
without a GPU: the weights of the three cubic filters are what their polynomials promise, with the bilinear tap the
statement is viewport_ref's bit for bit, Catmull-Rom on texel centres returns the texels, the overshoot case does leave
[0, 255] before the clamp -- and the four entry points are there and refuse a NULL frame."""
import ctypes as C

import numpy as np
import pytest

import chain_ref
import filter_ref
import viewport_ref
import warp_ref
from filter_ref import BILINEAR, BSPLINE, CATMULL_ROM, CUBIC, MITCHELL
from videomorphing_amd import capi, morph, synth
from videomorphing_amd.viewport import Viewport

f32 = np.float32
SHAPES = [(5, 3, 2), (33, 7, 3), (203, 77, 9)]
NAMES = ("vm_frame_render_viewport_filtered", "vm_frame_render_viewport_filtered_dev", "vm_frame_render_viewport_filtered_layers",
         "vm_frame_render_viewport_filtered_layers_dev")


def _bits(a, b):
    """bit for bit, a NaN for a NaN"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def test_the_constants_are_the_headers():
    assert (capi.FILTER_BILINEAR, capi.FILTER_CATMULL_ROM, capi.FILTER_MITCHELL, capi.FILTER_BSPLINE) == (0, 1, 2, 3)
    assert (BILINEAR, CATMULL_ROM, MITCHELL, BSPLINE) == (0, 1, 2, 3)
    for filt in CUBIC:
        assert len(filter_ref.COEFFS[filt]) == 7 and all(type(c) is np.float32 for c in filter_ref.COEFFS[filt])


def test_catmull_rom_weights_at_zero_are_the_texel():
    w = filter_ref.weights(f32(0), CATMULL_ROM)
    assert [float(t) for t in w] == [0.0, 1.0, 0.0, 0.0]


def test_the_step_overshoots_as_the_header_says():
    """a 0 / 255 step tapped at a = 0.25: 272.93 and -17.93 under Catmull-Rom, 260.98 and -5.98 under Mitchell, nothing
    outside [0, 255] under the B-spline"""
    for filt, hi, lo in ((CATMULL_ROM, 272.93, -17.93), (MITCHELL, 260.98, -5.98)):
        w = [float(t) for t in filter_ref.weights(f32(0.25), filt)]
        assert abs(255 * (w[1] + w[2] + w[3]) - hi) < 0.01 and abs(255 * w[0] - lo) < 0.01, (filt, w)      # the step one texel ahead / behind
    # (to a rounding: Horner's rule on coefficients of at most 2 and d <= 2 is off by less than 2^-19, which is how far
    # below zero outer(2 - a) may come out next to a = 0)
    assert all(float(t.min()) >= -2.0 ** -19 for t in filter_ref.weights(np.arange(65536, dtype=f32) / f32(65536), BSPLINE))


@pytest.mark.parametrize("filt", CUBIC)
def test_the_weights_sum_to_one(filt):
    """|sum - 1| <= 2^-19 over a = k / 65536 and over 2^20 random fractions (observed: at most 8 * 2^-23)"""
    rng = np.random.RandomState(5)
    for a in (np.arange(65536, dtype=f32) / f32(65536), rng.rand(1 << 20).astype(f32)):
        assert a.max() < 1
        w = filter_ref.weights(a, filt)
        total = ((w[0] + w[1]) + w[2]) + w[3]
        assert total.dtype == f32 and np.abs(total.astype(np.float64) - 1.0).max() <= 2.0 ** -19


def _canvases(w, h, ex):
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    return morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), rgb0, rgb1


@pytest.mark.parametrize("kind", ["smooth", "outside", "nan"])
def test_with_the_bilinear_tap_it_is_the_viewport_statement(kind):
    w, h, ex = 33, 7, 3
    e0, e1, rgb0, rgb1 = _canvases(w, h, ex)
    rng = np.random.RandomState(41)
    v, u = warp_ref.field(kind, w, h, rng), warp_ref.path(w, h, rng)
    l0, l1 = rgb0.astype(f32) / f32(3), rgb1.astype(f32) / f32(7)
    for vp in ((0.0, 0.0, 1.0, 1.0, w, h, 1, 1), (2.25, 0.5, 0.4, 0.4, 21, 9, 3, 2), (0.0, 0.0, 2.0, 2.0, 17, 4, 2, 2)):
        maps = viewport_ref.sample_maps(v, u, 0.3, vp)
        ok = chain_ref.founded(maps)
        for cf in (0, 1, 2):
            got = filter_ref.render_viewport_bytes(e0, e1, ex, maps, 0.3, cf, BILINEAR)
            want = viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.3, 0.3, cf, vp, maps)
            assert np.array_equal(got[ok], want[ok]), (vp, cf)
            assert _bits(filter_ref.layers_on_maps(l0, l1, maps, 0.3, cf, BILINEAR), viewport_ref.layers_on_maps(l0, l1, maps, 0.3, cf))
            assert _bits(filter_ref.layers_on_maps(l0[..., 0], l1[..., 0], maps, 0.3, cf, BILINEAR),
                         viewport_ref.layers_on_maps(l0[..., 0], l1[..., 0], maps, 0.3, cf))


@pytest.mark.parametrize("w,h,ex", SHAPES)
def test_catmull_rom_on_the_identity_viewport_of_a_zero_field_returns_the_image(w, h, ex):
    """every sample stands on a texel centre: the weights are (0, 1, 0, 0) in x and y, and 0 * t + 1 * t is t"""
    e0, e1, rgb0, rgb1 = _canvases(w, h, ex)
    zero = np.zeros((h, w, 2), f32)
    maps = viewport_ref.sample_maps(zero, None, 0.3, Viewport.identity(w, h).astuple())
    assert np.array_equal(filter_ref.render_viewport_bytes(e0, e1, ex, maps, 0.3, 0, CATMULL_ROM), rgb0)
    assert np.array_equal(filter_ref.render_viewport_bytes(e0, e1, ex, maps, 0.3, 2, CATMULL_ROM), rgb1)
    lay = (rgb0.astype(f32) + f32(1)) * f32(-1.75)      # (no zeros: +0 + -0 is +0)
    assert _bits(filter_ref.layers_on_maps(lay, lay, maps, 0.3, 0, CATMULL_ROM), lay)


def test_the_tap_never_reads_outside_the_image():
    """NaN, +-inf and 1e30 as coordinates: the float clamp stands before the conversion (numpy would raise on an index
    outside the image)"""
    img = np.arange(5 * 3 * 2, dtype=f32).reshape(3, 5, 2)
    bad = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 31, -2.0 ** 31, 2.5], f32)
    for filt in CUBIC:
        out = filter_ref.tap(img, bad, bad[::-1].copy(), filt)
        assert out.shape == (8, 2)
        far = filter_ref.tap(img, np.array([1e30, -1e30], f32), np.array([1.5, 1.5], f32), filt)
        # a finite coordinate far outside: floor(x) is x, a is 0, the four columns are the edge column
        assert np.isfinite(far).all()


@pytest.mark.parametrize("w,h,ex", SHAPES)
def test_the_overshoot_case_overshoots(w, h, ex):
    """the condition on the case that tests the clamp: before it, the mean goes below 0 in at least one pixel and above
    255 in at least one, under Catmull-Rom and Mitchell; the bytes there are 0 and 255; the B-spline stays inside to a rounding"""
    rgb, v, vp = filter_ref.overshoot_case(w, h)
    e = morph.make_extended(rgb, ex)
    maps = viewport_ref.sample_maps(v, None, 0.3, vp)
    for filt in (CATMULL_ROM, MITCHELL):
        mean = filter_ref.canvas_mean(e, e, ex, maps, 0.3, 0, filt)
        assert mean.shape == (h - 1, w - 1, 3) and (mean < 0).any() and (mean > 255).any(), (filt, float(mean.min()), float(mean.max()))
        out = chain_ref.bytes_of(mean, filt in CUBIC)
        assert np.all(out[mean < 0] == 0) and np.all(out[mean > 255] == 255)
    mean = filter_ref.canvas_mean(e, e, ex, maps, 0.3, 0, BSPLINE)
    # (sixteen products of weights that are off by less than 2^-19 each with texels of at most 255: 16 * 255 * 2^-19 < 0.01)
    assert mean.min() >= -0.01 and mean.max() <= 255.01


def test_the_entry_points_exist(vmlib):
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        assert hasattr(vmlib, n), "libvmorph_hip.so does not export %s" % n
    for n in ("render_viewport_filtered", "render_viewport_filtered_dev", "render_viewport_filtered_layers",
              "render_viewport_filtered_layers_dev"):
        assert callable(getattr(morph.Frame, n))


def test_a_null_frame_is_refused(vmlib):
    buf = C.create_string_buffer(64)
    ms = C.c_float(0)
    vp = Viewport.identity(2, 2).struct()
    assert vmlib.vm_frame_render_viewport_filtered(None, C.byref(vp), 1, 0.5, 0.5, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_frame_render_viewport_filtered:" in vmlib.vm_last_error()
    assert vmlib.vm_frame_render_viewport_filtered_dev(None, C.byref(vp), 1, 0.5, 0.5, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_frame_render_viewport_filtered_dev:" in vmlib.vm_last_error()
    assert vmlib.vm_frame_render_viewport_filtered_layers(None, C.byref(vp), 1, 0.5, 0.5, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_frame_render_viewport_filtered_layers:" in vmlib.vm_last_error()
    assert vmlib.vm_frame_render_viewport_filtered_layers_dev(None, C.byref(vp), 1, 0.5, 0.5, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_frame_render_viewport_filtered_layers_dev:" in vmlib.vm_last_error()
