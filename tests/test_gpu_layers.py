"""The warp kernels (videomorphing_amd/csrc/vm_warp.hip) behind vm_frame_sampling_maps, vm_frame_upload_layers and
vm_render_layers: bit for bit the float32 statement of tests/warp_ref.py, and anchored to the renderer that exists --
the GPU's maps, sampled on the host, give vm_render_halfway's bytes, and RGB carried as float layers rounds to them.

Shapes: 203x77 is no multiple of the 32x16 tile, 33x7 one partial tile narrower than the LDS window, 5x3 smaller than
the window's margin (every clamp), 138x84 the smoke shape.  Fields: those of test_render_window_hard_cases and the
smooth one, each with and without a path; the field with NaN / Inf in it is compared NaN for NaN and bit for bit
elsewhere (and must not fault)."""
import ctypes as C
import functools

import numpy as np
import pytest

import warp_ref
from render_cases import field as _field, rgb_pair as _rgb, same_bits as _same
from videomorphing_amd import capi, morph

pytestmark = pytest.mark.gpu

f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "rough", "large", "shear", "outside", "nan"]
FINITE = KINDS[:-1]
GEOS = (0.0, 0.2, 0.5, 1.0)
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)


@functools.lru_cache(maxsize=None)
def _ref_maps(w, h, kind, with_path, geo):
    """the statement's maps: computed once, shared, never written"""
    out = warp_ref.sampling_maps(*_field(w, h, kind, with_path), geo)
    for a in out:
        a.setflags(write=False)
    return out


def _frame(gpu_ctx, w, h, ex, kind, with_path, canvases=True):
    v, u = _field(w, h, kind, with_path)
    fr = morph.Frame(gpu_ctx, w, h, ex)
    if canvases:
        rgb0, rgb1 = _rgb(w, h)
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u)
    else:
        fr.upload(None, None, v, u)
    return fr


@shapes
@pytest.mark.parametrize("kind", KINDS)
@cases
def test_sampling_maps_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    """a: all four outputs, bit for bit, at geo_fa 0, 0.2, 0.5, 1; an output passed as NULL leaves the others what they are"""
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path, canvases=False)
    names = ("map0", "map1", "resid", "flags")
    for geo in GEOS:
        got = fr.sampling_maps(geo)
        want = _ref_maps(w, h, kind, with_path, geo)
        for n, g, r in zip(names, got, want):
            assert _same(g, r), (n, geo, int((g != r).sum()))
    # each output alone, and each one left out
    geo = 0.2
    want = _ref_maps(w, h, kind, with_path, geo)
    for mask in (1, 2, 4, 8, 14, 13, 11, 7):
        bufs = [np.full(r.shape, 77, r.dtype) for r in want]
        ptrs = [b.ctypes.data if mask >> k & 1 else None for k, b in enumerate(bufs)]
        capi.check(fr._L.vm_frame_sampling_maps(fr._h, geo, *ptrs))
        for k, (b, r) in enumerate(zip(bufs, want)):
            assert _same(b, r) if mask >> k & 1 else np.all(b == 77), (mask, names[k])
    fr.close()


@shapes
@pytest.mark.parametrize("kind", FINITE)
@cases
def test_maps_sampled_on_the_host_give_the_renderers_bytes(gpu_ctx, w, h, ex, kind, with_path):
    """b: the GPU's maps, the canvases the frame holds (download_ext) and the statement's tap, blend, + 0.5 and truncation
    on the host: vm_render_halfway's bytes, for color_from 0, 1, 2"""
    assert ex > 0
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    for geo in GEOS:
        m0, m1, _, _ = fr.sampling_maps(geo)
        for cf in (0, 1, 2):
            out = warp_ref.render_bytes(e0, e1, ex, m0, m1, 0.3, cf)
            ref = fr.render_halfway(0.3, geo, cf)
            assert np.array_equal(out, ref), (geo, cf, int((out != ref).sum()))
    fr.close()


@shapes
@pytest.mark.parametrize("kind", FINITE)
@cases
def test_rgb_as_float_layers_rounds_to_the_renderers_bytes(gpu_ctx, w, h, ex, kind, with_path):
    """c: a frame without an extension whose canvases are the two frames, and the same RGB as 3-channel float layers:
    (uint8)(double(render_layers) + 0.5) is vm_render_halfway's byte everywhere -- both clamp where a tap leaves the
    image, and the renderer's + 0.0f is exact"""
    fr = _frame(gpu_ctx, w, h, 0, kind, with_path)
    rgb0, rgb1 = _rgb(w, h)
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))
    for geo in GEOS:
        for cf in (0, 1, 2):
            lay = fr.render_layers(0.3, geo, cf)
            assert lay.shape == (h, w, 3) and lay.dtype == np.float32
            out = (lay.astype(np.float64) + 0.5).astype(np.uint8)
            ref = fr.render_halfway(0.3, geo, cf)
            assert np.array_equal(out, ref), (geo, cf, int((out != ref).sum()))
    fr.close()


def _layers(w, h, c, seed):
    """values of both signs over twelve orders of magnitude, +-1e6 among them"""
    rng = np.random.RandomState(seed)
    a = (rng.randn(h, w, c) * 10.0 ** rng.randint(-6, 6, (h, w, c))).astype(f32)
    a[rng.rand(h, w, c) < 0.05] = f32(1e6)
    a[rng.rand(h, w, c) < 0.05] = f32(-1e6)
    return a


@shapes
@pytest.mark.parametrize("kind", KINDS)
@cases
def test_render_layers_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    """d: 1, 2, 3 and 4 channels, color_from 0, 1, 2, bit for bit; a pitched output keeps what lies beyond its rows"""
    fr = _frame(gpu_ctx, w, h, ex, kind, with_path, canvases=False)
    for c in (1, 2, 3, 4):
        l0, l1 = _layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)
        if c == 1:
            l0, l1 = l0[..., 0], l1[..., 0]        # the (h, w) form
        fr.upload_layers(l0, l1)
        for geo in (0.2, 1.0):
            m0, m1, _, _ = _ref_maps(w, h, kind, with_path, geo)
            for cf in (0, 1, 2):
                got = fr.render_layers(0.3, geo, cf)
                want = warp_ref.render_layers(l0, l1, m0, m1, 0.3, cf)
                assert _same(got, want), (c, geo, cf, int((got != want).sum()))
        # rows of w * c floats in a pitch of w * c + 5
        pitch, sentinel = w * c + 5, f32(-12345.5)
        buf = np.full((h, pitch), sentinel, f32)
        capi.check(fr._L.vm_render_layers(fr._h, 0.3, 1.0, 1, buf.ctypes.data, pitch))
        want = warp_ref.render_layers(l0, l1, *_ref_maps(w, h, kind, with_path, 1.0)[:2], 0.3, 1)
        assert _same(buf[:, :w * c].reshape(want.shape), want) and np.all(buf[:, w * c:] == sentinel)
    fr.close()


def test_state_and_errors(gpu_ctx):
    """e: VM_E_STATE before an upload, re-upload with another channel count, every VM_E_INVALID, a positive time, and a
    frame that is what it was after all of it"""
    w, h, ex = 33, 7, 3
    fr = _frame(gpu_ctx, w, h, ex, "rough", True)
    L, hnd = fr._L, fr._h
    v0, q0, img0 = fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1)
    out = np.zeros((h, w, 4), f32)
    ms = C.c_float(-1.0)
    assert L.vm_render_layers(hnd, 0.3, 0.5, 1, out.ctypes.data, 0) == capi.VM_E_STATE
    assert L.vm_render_layers_dev(hnd, 0.3, 0.5, 1, C.byref(ms)) == capi.VM_E_STATE
    with pytest.raises(capi.VmError) as e:
        fr.render_layers(0.3, 0.5, 1)
    assert e.value.code == capi.VM_E_STATE
    l0, l1 = _layers(w, h, 4, 1), _layers(w, h, 4, 2)
    p0, p1 = l0.ctypes.data, l1.ctypes.data
    for ch in (0, 5, -1):
        assert L.vm_frame_upload_layers(hnd, ch, p0, p1, 0) == capi.VM_E_INVALID
    assert L.vm_frame_upload_layers(hnd, 2, None, p1, 0) == capi.VM_E_INVALID
    assert L.vm_frame_upload_layers(hnd, 2, p0, None, 0) == capi.VM_E_INVALID
    assert L.vm_frame_upload_layers(hnd, 2, p0, p1, 2 * w - 1) == capi.VM_E_INVALID
    assert L.vm_frame_upload_layers(hnd, 2, p0, p1, -4) == capi.VM_E_INVALID
    assert L.vm_render_layers(hnd, 0.3, 0.5, 1, out.ctypes.data, 0) == capi.VM_E_STATE      # refused uploads left no layers
    assert L.vm_frame_sampling_maps(hnd, 0.5, None, None, None, None) == capi.VM_E_INVALID
    # a pitched upload of 2 channels out of the 4-channel arrays, then 4 channels: the later upload wins
    m0, m1, _, _ = warp_ref.sampling_maps(*_field(w, h, "rough", True), 0.5)
    capi.check(L.vm_frame_upload_layers(hnd, 2, p0, p1, 4 * w))
    out2 = np.zeros((h, w, 2), f32)
    capi.check(L.vm_render_layers(hnd, 0.3, 0.5, 1, out2.ctypes.data, 0))
    assert _same(out2, warp_ref.render_layers(l0.reshape(h, 2 * w, 2)[:, :w], l1.reshape(h, 2 * w, 2)[:, :w], m0, m1, 0.3, 1))
    fr.upload_layers(l0, l1)
    assert _same(fr.render_layers(0.3, 0.5, 1), warp_ref.render_layers(l0, l1, m0, m1, 0.3, 1))
    for cf in (-1, 3):
        assert L.vm_render_layers(hnd, 0.3, 0.5, cf, out.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_layers_dev(hnd, 0.3, 0.5, cf, C.byref(ms)) == capi.VM_E_INVALID
    assert L.vm_render_layers(hnd, 0.3, 0.5, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_layers(hnd, 0.3, 0.5, 1, out.ctypes.data, 4 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_layers(hnd, 0.3, 0.5, 1, out.ctypes.data, -1) == capi.VM_E_INVALID
    assert fr.render_layers_dev(0.3, 0.5, 1) > 0
    capi.check(L.vm_render_layers_dev(hnd, 0.3, 0.5, 1, None))
    fr.sampling_maps(0.5)
    assert np.array_equal(fr.download_v().view(np.uint32), v0.view(np.uint32))
    assert np.array_equal(fr.download_qpath().view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), img0)
    fr.close()
