"""tests/transit_shutter_ref.py, the numpy statement of a shutter under a transition schedule
(videomorphing_amd/csrc/vm_tshutter.hip), pinned without a GPU to the two statements it joins, bit for bit and a NaN for a
NaN: one sample at t_open == t_close == t_color == t is tests/transit_ref.py's transition call at t, for either ease and
any schedule; the schedule (0, 1) on both planes with the linear ease is tests/shutter_ref.py's uniform shutter at
color_fa = t_color.  And the entry points exist in the binding and the library and refuse a NULL frame."""
import ctypes as C
import functools

import numpy as np
import pytest

import chain_ref
import shutter_ref
from render_cases import same_bits as _same
import transit_ref
import transit_shutter_ref as TS
import warp_ref
from videomorphing_amd import capi, morph, synth, transition

f32 = np.float32
SHAPES = [(33, 7, 3), (5, 3, 2), (70, 40, 4)]
KINDS = ["smooth", "large", "outside", "nan"]
NAMES = ("vm_render_transition_shutter", "vm_render_transition_shutter_dev", "vm_render_transition_shutter_layers",
         "vm_render_transition_shutter_layers_dev")
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)
cases = pytest.mark.parametrize("with_path", [False, True])


@functools.lru_cache(maxsize=None)
def _case(w, h, ex, kind, with_path):
    rng = np.random.RandomState(41)
    v = warp_ref.field(kind, w, h, rng)
    u = warp_ref.path(w, h, rng) if with_path else None
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
    l0, l1 = rgb0.astype(f32) / f32(3), rgb1.astype(f32) / f32(7)
    return v, u, e0, e1, l0, l1


@shapes
@kinds
@cases
@pytest.mark.parametrize("ease", [transit_ref.EASE_LINEAR, transit_ref.EASE_SMOOTH])
def test_one_sample_is_the_transition_statement(w, h, ex, kind, with_path, ease):
    """N = 1 at t_open == t_close == t_color == t: t_0 = t + 0 * f is t, 0 + c is c and c / 1 is c"""
    v, u, e0, e1, l0, l1 = _case(w, h, ex, kind, with_path)
    sg, sc = transition.wipe(w, h), transition.radial(w, h)
    for t in (0.0, 0.3, 0.55, 1.0, 1.2):
        assert TS.sample_times(t, t, 1)[0].view(np.uint32) == f32(t).view(np.uint32)
        m0, m1, _, _, rates = transit_ref.transition_maps(v, u, sg, sc, t, ease)
        maps = TS.sample_maps(v, u, sg, sc, t, t, 1, t, ease)
        assert _same(maps[0][0], m0) and _same(maps[0][1], m1) and _same(maps[0][2], rates[..., 1]), t
        ok = chain_ref.founded(maps)
        assert kind == "nan" or ok.all()
        for cf in (0, 1, 2):
            got = chain_ref.bytes_of(TS.canvas_mean(e0, e1, ex, maps, cf))
            want = transit_ref.render_bytes(e0, e1, ex, m0, m1, rates[..., 1], cf)
            assert np.array_equal(got[ok], want[ok]), (t, cf)
            for a, b in ((l0, l1), (l0[..., 0], l1[..., 1])):
                got = TS.layers_on_maps(a, b, maps, cf)
                assert _same(got, transit_ref.render_layers(a, b, m0, m1, rates[..., 1], cf)), (t, cf)


@shapes
@kinds
@cases
def test_the_uniform_schedule_is_the_shutter_statement(w, h, ex, kind, with_path):
    """schedule (0, 1) on both planes, linear ease: G_s is the constant fminf(fmaxf(t_s, 0), 1), K the constant t_color,
    and a rate tap of a constant plane is that constant -- shutters inside the morph, across all of it, short, open
    across t = 0 and t = 1, and reversed"""
    v, u, e0, e1, l0, l1 = _case(w, h, ex, kind, with_path)
    for n, (o, c) in ((1, (0.4, 0.4)), (2, (0.7, 0.3)), (5, (0.0, 1.0)), (5, (0.50, 0.52)), (3, (-0.2, 0.2)), (4, (0.9, 1.2))):
        for tc in (0.3, 0.0, 1.0):
            if tc != 0.3 and n != 5:
                continue
            maps = TS.sample_maps(v, u, None, None, o, c, n, tc, transit_ref.EASE_LINEAR)
            want = shutter_ref.sample_maps(v, u, o, c, n)
            for (g0, g1, k), (w0, w1) in zip(maps, want):
                assert _same(g0, w0) and _same(g1, w1), (n, o, c)
                # (a position that is no number has no fractions, and its k is none either)
                at = np.isfinite(g0).all(-1) & np.isfinite(g1).all(-1)
                assert np.all(k[at].view(np.uint32) == f32(tc).view(np.uint32)) and np.all(np.isnan(k[~at]) | (k[~at] == f32(tc)))
            ok = chain_ref.founded(maps)
            assert kind == "nan" or ok.all()
            for cf in (0, 1, 2):
                got = chain_ref.bytes_of(TS.canvas_mean(e0, e1, ex, maps, cf))
                ref = chain_ref.bytes_of(shutter_ref.canvas_mean(e0, e1, ex, want, tc, cf))
                assert np.array_equal(got[ok], ref[ok]), (n, o, c, tc, cf)
                got = TS.layers_on_maps(l0, l1, maps, cf)
                assert _same(got, shutter_ref.layers_on_maps(l0, l1, want, tc, cf)), (n, o, c, tc, cf)


def test_sample_times_are_not_clamped():
    got = TS.sample_times(-0.4, 1.4, 4)
    o, d = f32(-0.4), f32(1.4) - f32(-0.4)
    assert got.dtype == np.float32
    assert np.array_equal(got, np.array([o + d * f32(f) for f in (0.125, 0.375, 0.625, 0.875)], f32))
    assert got[0] < 0 and got[-1] > 1
    # inside [0, 1] they are the uniform shutter's
    assert np.array_equal(TS.sample_times(0.3, 0.7, 5), shutter_ref.sample_times(0.3, 0.7, 5))
    for n in (0, 65):
        with pytest.raises(AssertionError):
            TS.sample_times(0.0, 1.0, n)


def test_a_moving_wipe_is_not_a_fixed_one():
    """the geometry schedule is ramped per sample: a shutter across a wipe differs from the mean under the rates of its
    middle, so a statement (or a kernel) that ramps G once cannot pass for this one"""
    w, h, ex = 70, 40, 4
    v, u, e0, e1, l0, l1 = _case(w, h, ex, "smooth", False)
    sg = transition.wipe(w, h)
    moving = TS.render_layers(l0, l1, v, u, sg, None, 0.3, 0.7, 4, 0.5, 0, 1)
    still = TS.render_layers(l0, l1, v, u, sg, None, 0.5, 0.5, 4, 0.5, 0, 1)
    assert not np.array_equal(moving, still)


def test_the_entry_points_exist(vmlib):
    for n in NAMES:
        assert n in capi.SYMBOLS, n
        assert hasattr(vmlib, n), "libvmorph_hip.so does not export %s" % n
    for n in ("render_transition_shutter", "render_transition_shutter_dev", "render_transition_shutter_layers",
              "render_transition_shutter_layers_dev"):
        assert callable(getattr(morph.Frame, n))


def test_a_null_frame_is_refused(vmlib):
    buf = C.create_string_buffer(64)
    ms = C.c_float(0)
    assert vmlib.vm_render_transition_shutter(None, 0.4, 0.6, 4, 0.5, 0, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_transition_shutter:" in vmlib.vm_last_error()
    assert vmlib.vm_render_transition_shutter_dev(None, 0.4, 0.6, 4, 0.5, 0, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_transition_shutter_dev:" in vmlib.vm_last_error()
    assert vmlib.vm_render_transition_shutter_layers(None, 0.4, 0.6, 4, 0.5, 0, 1, buf, 0) == capi.VM_E_INVALID
    assert b"vm_render_transition_shutter_layers:" in vmlib.vm_last_error()
    assert vmlib.vm_render_transition_shutter_layers_dev(None, 0.4, 0.6, 4, 0.5, 0, 1, C.byref(ms)) == capi.VM_E_INVALID
    assert b"vm_render_transition_shutter_layers_dev:" in vmlib.vm_last_error()


def test_the_default_colour_time_is_the_float32_midpoint():
    assert morph.Frame._shutter_color_time(0.4, 0.6, None) == float((f32(0.4) + f32(0.6)) * f32(0.5))
    assert morph.Frame._shutter_color_time(0.4, 0.6, 0.25) == 0.25
