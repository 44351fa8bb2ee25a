"""tests/shutter_ref.py, the numpy statement of the shutter calls (videomorphing_amd/csrc/vm_shutter.hip), pinned without a
GPU: one sample at one time is the uniform statement of tests/warp_ref.py, a zero field gives side 0's image whatever the
shutter, the sample times are the stated values -- and the entry points exist in the binding and the library and refuse
a NULL frame."""
import ctypes as C

import numpy as np
import pytest

import shutter_ref
import warp_ref
from videomorphing_amd import capi, morph, synth

f32 = np.float32
W, H, EX = 45, 23, 4
NAMES = ("vm_render_shutter", "vm_render_shutter_dev", "vm_render_shutter_layers", "vm_render_shutter_layers_dev")


def _case(with_path):
    rng = np.random.RandomState(7)
    v = warp_ref.field("smooth", W, H, rng)
    u = warp_ref.path(W, H, rng) if with_path else None
    rgb0, rgb1 = synth.make_rgb_pair(W, H)
    return v, u, rgb0, rgb1


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("with_path", [False, True])
def test_one_sample_is_the_uniform_statement(with_path):
    """N = 1 at open == close == g: t_0 is g, 0 + c is c and c / 1 is c"""
    v, u, rgb0, rgb1 = _case(with_path)
    e0, e1 = morph.make_extended(rgb0, EX), morph.make_extended(rgb1, EX)
    l0, l1 = rgb0.astype(f32) / f32(3), rgb1[..., 0].astype(f32) / f32(7)
    for g in (0.0, 0.3, 1.0):
        assert shutter_ref.sample_times(g, g, 1)[0] == f32(g)
        m0, m1, _, _ = warp_ref.sampling_maps(v, u, g)
        for cf in (0, 1, 2):
            got = shutter_ref.render_shutter_bytes(e0, e1, EX, v, u, 0.3, g, g, 1, cf)
            assert np.array_equal(got, warp_ref.render_bytes(e0, e1, EX, m0, m1, 0.3, cf)), (g, cf)
            got = shutter_ref.render_shutter_layers(l0, l0[::-1].copy(), v, u, 0.3, g, g, 1, cf)
            assert _same(got, warp_ref.render_layers(l0, l0[::-1].copy(), m0, m1, 0.3, cf)), (g, cf)
            got = shutter_ref.render_shutter_layers(l1, l1[:, ::-1].copy(), v, u, 0.3, g, g, 1, cf)
            assert _same(got, warp_ref.render_layers(l1, l1[:, ::-1].copy(), m0, m1, 0.3, cf)), (g, cf)


@pytest.mark.parametrize("n", [1, 3, 64])
def test_a_zero_field_gives_side_0s_image(n):
    """every tap lands on a texel, the sum of n <= 64 integers below 256 is exact and so is its division by n"""
    _, _, rgb0, rgb1 = _case(False)
    e0, e1 = morph.make_extended(rgb0, EX), morph.make_extended(rgb1, EX)
    v = np.zeros((H, W, 2), f32)
    for o, c in ((0.3, 0.7), (0.0, 1.0), (-0.2, 0.2), (0.7, 0.3)):
        assert np.array_equal(shutter_ref.render_shutter_bytes(e0, e1, EX, v, None, 0.3, o, c, n, 0), rgb0), (o, c)
        got = shutter_ref.render_shutter_layers(rgb0.astype(f32), rgb1.astype(f32), v, None, 0.3, o, c, n, 0)
        assert _same(got, rgb0.astype(f32)), (o, c)


def test_sample_times():
    def t(*a):
        out = shutter_ref.sample_times(*a)
        assert out.dtype == np.float32
        return out

    # f = 0.125, 0.375, 0.625, 0.875 (exact); 0.3f + 0.4f * f in float32
    o, d = f32(0.3), f32(0.7) - f32(0.3)
    want = np.array([o + d * f32(f) for f in (0.125, 0.375, 0.625, 0.875)], f32)
    assert np.array_equal(t(0.3, 0.7, 4), want)
    assert np.allclose(want, [0.35, 0.45, 0.55, 0.65], rtol=0, atol=1e-7)
    # open across t = 0: -0.16, -0.08 and 0 (to a rounding) hold at 0, then 0.08, 0.16
    got = t(-0.2, 0.2, 5)
    assert np.all(got[:2] == 0) and abs(got[2]) < 1e-7 and np.allclose(got[3:], [0.08, 0.16], rtol=0, atol=1e-7)
    assert np.all(got >= 0)
    # open across t = 1: 1.0 and 1.2 hold at 1
    assert np.array_equal(t(0.9, 1.3, 2), np.array([1, 1], f32))
    # the reversed interval runs backwards through (to a rounding) the same times
    back = t(0.7, 0.3, 4)
    assert np.all(np.diff(back) < 0) and np.allclose(back[::-1], want, rtol=0, atol=1e-7)
    assert t(0.25, 0.25, 1)[0] == f32(0.25)
    for n in (0, 65):
        with pytest.raises(AssertionError):
            shutter_ref.sample_times(0.0, 1.0, n)


def test_the_entry_points_exist(vmlib):
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        assert hasattr(vmlib, n), "libvmorph_hip.so does not export %s" % n
    for n in ("render_shutter", "render_shutter_dev", "render_shutter_layers", "render_shutter_layers_dev"):
        assert callable(getattr(morph.Frame, n))


def test_a_null_frame_is_refused(vmlib):
    buf = C.create_string_buffer(64)
    ms = C.c_float(0)
    assert vmlib.vm_render_shutter(None, 0.5, 0.4, 0.6, 4, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_shutter:" in vmlib.vm_last_error()
    assert vmlib.vm_render_shutter_dev(None, 0.5, 0.4, 0.6, 4, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_shutter_dev:" in vmlib.vm_last_error()
    assert vmlib.vm_render_shutter_layers(None, 0.5, 0.4, 0.6, 4, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_shutter_layers:" in vmlib.vm_last_error()
    assert vmlib.vm_render_shutter_layers_dev(None, 0.5, 0.4, 0.6, 4, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_shutter_layers_dev:" in vmlib.vm_last_error()
