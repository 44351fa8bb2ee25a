"""Transition control on the GPU (the RATES instantiations of videomorphing_amd/csrc/vm_warp.hip behind
vm_frame_upload_schedule, vm_render_transition, vm_render_transition_layers and vm_frame_transition_maps): tied to the
kernels that exist -- under the schedule (0, 1) every call gives the bits of its uniform counterpart -- and bit for bit
the float32 statement of tests/transit_ref.py under schedules that are not uniform.

Shapes and fields are those of tests/test_gpu_layers.py: 203x77 is no multiple of the 32x16 tile, 33x7 one partial tile
narrower than the LDS window, 5x3 smaller than the window's margin (every clamp), 138x84 the smoke shape; the large
field's taps leave the window, the field with NaN / Inf in it is compared NaN for NaN and bit for bit elsewhere (and must
not fault).  RGB8 bytes are compared where both sampling positions are finite: what a NaN becomes as a byte is defined
neither by C nor by numpy."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

import transit_ref
from render_cases import field as _field, hashes_under_render_mode, layers as _layers, rgb_pair as _rgb, same_bits as _same
from videomorphing_amd import capi, morph, transition

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "rough", "large", "shear", "outside", "nan"]
SCHEDULES = ["wipe", "radial", "step", "split"]
TIMES = (0.0, 0.3, 0.5, 0.7, 1.0)
EASES = (capi.EASE_LINEAR, capi.EASE_SMOOTH)
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)


@functools.lru_cache(maxsize=None)
def _schedule(w, h, name):
    """(geometry, colour): a soft wipe (lead, lead + 0.4), a radial one, a hard step t1 == t0, and a wipe for the
    geometry with a slower radial schedule for the colour"""
    if name == "wipe":
        s = transition.wipe(w, h, (1.0, 0.3), lead=0.6, duration=0.4)
        assert np.all(s[..., 1] - s[..., 0] > 0.39)
        out = s, s
    elif name == "radial":
        s = transition.radial(w, h, (0.3 * w, 0.6 * h), lead=0.5, duration=0.5)
        out = s, s
    elif name == "step":
        s = transition.wipe(w, h, (0.2, 1.0), lead=1.0, duration=0.0)
        assert np.array_equal(s[..., 0], s[..., 1])
        out = s, s
    else:
        out = transition.wipe(w, h, (-1.0, 0.5), lead=0.7, duration=0.3), transition.radial(w, h, None, lead=0.2, duration=0.8)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=48)
def _ref(w, h, kind, with_path, name, t, ease):
    """the statement's maps and rates: computed once per case, shared by its layer and byte checks, never written"""
    out = transit_ref.transition_maps(*_field(w, h, kind, with_path), *_schedule(w, h, name), t, ease)
    for a in out:
        a.setflags(write=False)
    return out


def _founded(m0, m1):
    """where a byte is defined: both sampling positions finite"""
    return np.isfinite(m0).all(-1) & np.isfinite(m1).all(-1)


def _frame(gpu_ctx, w, h, ex, kind, with_path):
    v, u = _field(w, h, kind, with_path)
    fr = morph.Frame(gpu_ctx, w, h, ex)
    rgb0, rgb1 = _rgb(w, h)
    fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u)
    return fr


@shapes
@pytest.mark.parametrize("kind", KINDS)
@cases
def test_uniform_schedule_gives_the_uniform_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """schedule (0, 1), linear ease, t = color_fa = geo_fa: vm_render_transition gives vm_render_halfway's bytes,
    vm_render_transition_layers vm_render_layers' bits and vm_frame_transition_maps vm_frame_sampling_maps' bits, for
    every color_from; one plane uploaded and one NULL, and the other way round"""
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path)
    uni = transition.uniform(w, h)
    fr.upload_layers(_layers(w, h, 4, 14), _layers(w, h, 4, 24))
    for k, t in enumerate((0.0, 0.2, 0.5, 1.0)):
        fr.upload_schedule(*((uni, None) if k % 2 else (None, uni)))
        got = fr.transition_maps(t)
        for n, g, r in zip(("map0", "map1", "resid", "flags"), got, fr.sampling_maps(t)):
            assert _same(g, r), (n, t, int((g != r).sum()))
        ok = _founded(got[0], got[1])
        assert kind == "nan" or ok.all()
        assert np.all(got[4][ok].view(np.uint32) == f32(t).view(np.uint32)), t
        for cf in (0, 1, 2):
            out, ref = fr.render_transition(t, capi.EASE_LINEAR, cf), fr.render_halfway(t, t, cf)
            assert np.array_equal(out[ok], ref[ok]), (t, cf, int((out != ref).sum()))
            assert kind != "nan" or np.array_equal(out, ref)           # (the same conversion in both kernels)
            lay, ref = fr.render_transition_layers(t, capi.EASE_LINEAR, cf), fr.render_layers(t, t, cf)
            assert _same(lay, ref), (t, cf, int((lay != ref).sum()))
    fr.close()


@shapes
@pytest.mark.parametrize("kind", ["smooth", "rough", "large", "outside", "nan"])
@cases
def test_scheduled_calls_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    """four schedules, t in 0, 0.3, 0.5, 0.7, 1, both eases: the maps, rates_gk, the layers for 1 and 3 channels and the
    RGB8 bytes, bit for bit; every color_from at one of the times; each output of the maps call alone"""
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    names = ("map0", "map1", "resid", "flags", "rates")
    for c in (1, 3):
        l0, l1 = _layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)
        fr.upload_layers(l0, l1)
        for name in SCHEDULES:
            fr.upload_schedule(*_schedule(w, h, name))
            for t in TIMES:
                for ease in EASES:
                    want = _ref(w, h, kind, with_path, name, t, ease)
                    m0, m1, k = want[0], want[1], want[4][..., 1]
                    for cf in ((0, 1, 2) if t == 0.3 else (1,)):
                        got = fr.render_transition_layers(t, ease, cf)
                        ref = transit_ref.render_layers(l0, l1, m0, m1, k, cf)
                        assert _same(got, ref), (c, name, t, ease, cf, int((got != ref).sum()))
                    if c != 1:
                        continue
                    got = fr.transition_maps(t, ease)
                    for n, g, r in zip(names, got, want):
                        assert _same(g, r), (n, name, t, ease, int((g != r).sum()))
                    ok = _founded(m0, m1)
                    assert kind == "nan" or ok.all()
                    for cf in ((0, 1, 2) if t == 0.3 else (1,)):
                        got = fr.render_transition(t, ease, cf)
                        ref = transit_ref.render_bytes(e0, e1, ex, m0, m1, k, cf)
                        assert np.array_equal(got[ok], ref[ok]), (name, t, ease, cf, int((got != ref).sum()))
    # each output alone, and each one left out
    t, ease = 0.5, capi.EASE_SMOOTH
    want = _ref(w, h, kind, with_path, SCHEDULES[-1], t, ease)
    for mask in (1, 2, 4, 8, 16, 30, 29, 27, 23, 15):
        bufs = [np.full(r.shape, 77, r.dtype) for r in want]
        ptrs = [b.ctypes.data if mask >> k & 1 else None for k, b in enumerate(bufs)]
        capi.check(fr._L.vm_frame_transition_maps(fr._h, t, ease, *ptrs))
        for k, (b, r) in enumerate(zip(bufs, want)):
            assert _same(b, r) if mask >> k & 1 else np.all(b == 77), (mask, names[k])
    fr.close()


@pytest.mark.parametrize("w,h,ex", [(203, 77, 9), (138, 84, 8)])
def test_two_halves_equal_the_uniform_extremes_away_from_the_seam(gpu_ctx, w, h, ex):
    """the left half scheduled (0, 0.5), the right half (0.5, 1), t = 0.5: every output column at least
    ceil(max|v.x|) + 2 from the seam has the bits of vm_frame_sampling_maps at geo_fa = 1 (left) and 0 (right), for
    both eases; the band between differs from both"""
    fr = _frame(gpu_ctx, w, h, ex, "smooth", True)
    v, _ = _field(w, h, "smooth", True)
    left, right = transit_ref.two_halves_columns(v, w)
    assert 4 * (len(left) + len(right)) >= 3 * w
    band = np.arange(left[-1] + 1, right[0])
    one, zero = fr.sampling_maps(1.0), fr.sampling_maps(0.0)
    fr.upload_schedule(transit_ref.two_halves(w, h), None)
    for ease in EASES:
        got = fr.transition_maps(0.5, ease)
        for n, g, a, b in zip(("map0", "map1", "resid", "flags"), got, one, zero):
            assert _same(g[:, left], a[:, left]), (n, ease, "left")
            assert _same(g[:, right], b[:, right]), (n, ease, "right")
        for a in (one, zero):
            assert not np.array_equal(got[0][:, band], a[0][:, band])
    fr.close()


@shapes
@pytest.mark.parametrize("kind", ["smooth", "rough", "large", "shear", "outside"])
@cases
def test_transition_maps_sampled_on_the_host_give_the_rendered_bytes(gpu_ctx, w, h, ex, kind, with_path):
    """the GPU's maps and k, the canvases the frame holds and the statement's tap, blend, + 0.5 and truncation on the
    host: vm_render_transition's bytes, for color_from 0, 1, 2"""
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    fr.upload_schedule(*_schedule(w, h, "split"))
    for t, ease in ((0.3, capi.EASE_LINEAR), (0.5, capi.EASE_SMOOTH), (0.7, capi.EASE_LINEAR)):
        m0, m1, _, _, rates = fr.transition_maps(t, ease)
        for cf in (0, 1, 2):
            out = transit_ref.render_bytes(e0, e1, ex, m0, m1, rates[..., 1], cf)
            ref = fr.render_transition(t, ease, cf)
            assert np.array_equal(out, ref), (t, ease, cf, int((out != ref).sum()))
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from videomorphing_amd import capi, morph, synth, transition
    w, h, ex = 203, 77, 9
    rng = np.random.RandomState(41)
    v, u = warp_ref.field("rough", w, h, rng), warp_ref.path(w, h, rng)
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    fr = morph.Frame(morph.Context(0, capi.MATH_FAST), w, h, ex)
    hh = hashlib.sha256()
    for path in (None, u):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, path)
        fr.upload_layers(rgb0.astype(np.float32), rgb1.astype(np.float32))
        fr.upload_schedule(transition.wipe(w, h, (-1.0, 0.5), lead=0.7, duration=0.3), transition.radial(w, h, None, lead=0.2, duration=0.8))
        for t, ease in ((0.3, 0), (0.7, 1)):
            for a in fr.transition_maps(t, ease):
                hh.update(a.tobytes())
            hh.update(fr.render_transition(t, ease, 1).tobytes())
            hh.update(fr.render_transition_layers(t, ease, 1).tobytes())
    print("HASH", hh.hexdigest())
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain -- also the path of fields of 4 GiB and more) give the window kernels'
    bits: a fresh child process with the switch set hashes the maps, the bytes and the layers of two scheduled calls
    with and without a path, another one hashes the window form's"""
    assert hashes_under_render_mode(_PROG, "plain")[0] == hashes_under_render_mode(_PROG, None)[0]


def test_state_and_errors(gpu_ctx):
    """VM_E_STATE without a schedule, after clearing it and without layers; re-upload with one plane NULL; every
    VM_E_INVALID; a positive time; and a frame that is what it was after all of it"""
    w, h, ex = 33, 7, 3
    fr = _frame(gpu_ctx, w, h, ex, "rough", True)
    L, hnd = fr._L, fr._h
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    fr.upload_layers(l0, l1)
    v0, q0, img0, lay0 = fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1)
    rgb, out, ms = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 2), f32), C.c_float(-1.0)
    maps = [np.zeros((h, w, 2), f32), np.zeros((h, w, 2), f32), np.zeros((h, w), f32), np.zeros((h, w), np.uint8), np.zeros((h, w, 2), f32)]
    mp = [m.ctypes.data for m in maps]

    def no_schedule():
        assert L.vm_render_transition(hnd, 0.5, 0, 1, rgb.ctypes.data, 0) == capi.VM_E_STATE
        assert L.vm_render_transition_dev(hnd, 0.5, 0, 1, C.byref(ms)) == capi.VM_E_STATE
        assert L.vm_render_transition_layers(hnd, 0.5, 0, 1, out.ctypes.data, 0) == capi.VM_E_STATE
        assert L.vm_render_transition_layers_dev(hnd, 0.5, 0, 1, C.byref(ms)) == capi.VM_E_STATE
        assert L.vm_frame_transition_maps(hnd, 0.5, 0, *mp) == capi.VM_E_STATE
        with pytest.raises(capi.VmError) as e:
            fr.render_transition(0.5)
        assert e.value.code == capi.VM_E_STATE

    no_schedule()
    sg, sk = _schedule(w, h, "split")
    assert L.vm_frame_upload_schedule(hnd, None, None, 0) == capi.VM_E_INVALID
    assert L.vm_frame_upload_schedule(hnd, sg.ctypes.data, sk.ctypes.data, 2 * w - 1) == capi.VM_E_INVALID
    assert L.vm_frame_upload_schedule(hnd, sg.ctypes.data, sk.ctypes.data, -2) == capi.VM_E_INVALID
    no_schedule()                                       # refused uploads left no schedule
    fr.upload_schedule(sg, sk)
    v, u = _field(w, h, "rough", True)
    want = transit_ref.transition_maps(v, u, sg, sk, 0.5, 1)
    assert all(_same(g, r) for g, r in zip(fr.transition_maps(0.5, 1), want))
    fr.clear_schedule()
    no_schedule()
    # re-upload with one plane NULL (uniform colour), out of a pitched array
    pitch = 2 * w + 6
    wide = np.full((h, pitch), 9.0, f32)
    wide[:, :2 * w] = sg.reshape(h, 2 * w)
    capi.check(L.vm_frame_upload_schedule(hnd, wide.ctypes.data, None, pitch))
    want = transit_ref.transition_maps(v, u, sg, None, 0.5, 1)
    assert all(_same(g, r) for g, r in zip(fr.transition_maps(0.5, 1), want))
    fr.upload_schedule(sg, sk)                          # the later upload wins
    want = transit_ref.transition_maps(v, u, sg, sk, 0.3, 0)
    assert all(_same(g, r) for g, r in zip(fr.transition_maps(0.3, 0), want))
    # pitched outputs keep what lies beyond their rows
    big = np.full((h, 3 * w + 5), 201, np.uint8)
    capi.check(L.vm_render_transition(hnd, 0.3, 0, 1, big.ctypes.data, 3 * w + 5))
    assert np.array_equal(big[:, :3 * w].reshape(h, w, 3), fr.render_transition(0.3, 0, 1)) and np.all(big[:, 3 * w:] == 201)
    bigf = np.full((h, 2 * w + 3), f32(-12345.5), f32)
    capi.check(L.vm_render_transition_layers(hnd, 0.3, 0, 1, bigf.ctypes.data, 2 * w + 3))
    ref = transit_ref.render_layers(l0, l1, want[0], want[1], want[4][..., 1], 1)
    assert _same(bigf[:, :2 * w].reshape(h, w, 2), ref) and np.all(bigf[:, 2 * w:] == f32(-12345.5))
    for ease in (-1, 2):
        assert L.vm_render_transition(hnd, 0.5, ease, 1, rgb.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_transition_dev(hnd, 0.5, ease, 1, C.byref(ms)) == capi.VM_E_INVALID
        assert L.vm_render_transition_layers(hnd, 0.5, ease, 1, out.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_transition_layers_dev(hnd, 0.5, ease, 1, C.byref(ms)) == capi.VM_E_INVALID
        assert L.vm_frame_transition_maps(hnd, 0.5, ease, *mp) == capi.VM_E_INVALID
    for cf in (-1, 3):
        assert L.vm_render_transition(hnd, 0.5, 0, cf, rgb.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_transition_dev(hnd, 0.5, 0, cf, C.byref(ms)) == capi.VM_E_INVALID
        assert L.vm_render_transition_layers(hnd, 0.5, 0, cf, out.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_transition_layers_dev(hnd, 0.5, 0, cf, C.byref(ms)) == capi.VM_E_INVALID
    assert L.vm_render_transition(hnd, 0.5, 0, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_transition(hnd, 0.5, 0, 1, rgb.ctypes.data, 3 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_transition(hnd, 0.5, 0, 1, rgb.ctypes.data, -1) == capi.VM_E_INVALID
    assert L.vm_render_transition_layers(hnd, 0.5, 0, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_transition_layers(hnd, 0.5, 0, 1, out.ctypes.data, 2 * w - 1) == capi.VM_E_INVALID
    assert L.vm_frame_transition_maps(hnd, 0.5, 0, None, None, None, None, None) == capi.VM_E_INVALID
    assert fr.render_transition_dev(0.5) > 0 and fr.render_transition_layers_dev(0.5) > 0
    capi.check(L.vm_render_transition_dev(hnd, 0.5, 0, 1, None))
    # a frame with a schedule and no layers
    bare = _frame(gpu_ctx, w, h, ex, "rough", False)
    bare.upload_schedule(sg, None)
    assert L.vm_render_transition_layers(bare._h, 0.5, 0, 1, out.ctypes.data, 0) == capi.VM_E_STATE
    assert L.vm_render_transition_layers_dev(bare._h, 0.5, 0, 1, C.byref(ms)) == capi.VM_E_STATE
    bare.render_transition(0.5)
    bare.close()
    # the frame is what it was
    assert np.array_equal(fr.download_v().view(np.uint32), v0.view(np.uint32))
    assert np.array_equal(fr.download_qpath().view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), img0)
    assert _same(fr.render_layers(0.3, 0.35, 1), lay0)
    fr.close()
