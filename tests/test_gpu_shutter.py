"""The shutter kernels (videomorphing_amd/csrc/vm_shutter.hip) behind vm_render_shutter and vm_render_shutter_layers: tied
to the kernels that exist -- one sample at one time gives vm_render_halfway's bytes and vm_render_layers' bits -- and bit
for bit the float32 statement of tests/shutter_ref.py for N in 2, 5, 16 under shutters inside the morph, across all of it,
short, open across t = 0, and reversed.

Shapes are those of tests/test_gpu_layers.py: 203x77 is no multiple of the 32x16 tile, 33x7 one partial tile narrower
than the LDS window (half of its waves have no pixel and are in the loop for the barriers alone), 5x3 smaller than the
window's margin, 138x84 the smoke shape.  Fields: smooth, large, outside and the one with NaN / Inf in it (compared NaN for
NaN, and must not fault).  Under the shutter (0, 1) the large field moves the window by about 110 px from sample to
sample, so a missing restage or barrier shows; under (0.50, 0.52) consecutive windows coincide.

Every shape takes every N with every shutter against the statement, which walks the chain once per sample time in numpy
(about 0.1 s at 203x77: 115 sample times a case, those that occur twice walked once).  That is some ten seconds for a
case of the two multi-tile shapes -- the price of holding N = 16 with a moving window to the statement where there is more
than one tile.  RGB8 bytes are compared where every sample's two positions are finite: what a NaN
becomes as a byte is defined neither by C nor by numpy."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

import chain_ref
import shutter_ref
from render_cases import field as _field, frame as _frame, hashes_under_render_mode, layers as _layers, rgb_pair as _rgb, same_bits as _same
import warp_ref
from videomorphing_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "large", "outside", "nan"]
NS = (2, 5, 16)
SHUTTERS = ((0.3, 0.7), (0.0, 1.0), (0.50, 0.52), (-0.2, 0.2), (0.7, 0.3))
EVERY = [(n, sh) for n in NS for sh in SHUTTERS]
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)


@functools.lru_cache(maxsize=128)
def _maps_at(w, h, kind, with_path, t_bits):
    """the statement's (map0, map1) at one sample time: computed once, shared, never written"""
    out = warp_ref.sampling_maps(*_field(w, h, kind, with_path), np.uint32(t_bits).view(f32))[:2]
    for a in out:
        a.setflags(write=False)
    return out


def _ref_maps(w, h, kind, with_path, o, c, n):
    return [_maps_at(w, h, kind, with_path, int(t.view(np.uint32))) for t in shutter_ref.sample_times(o, c, n)]


@shapes
@kinds
@cases
def test_one_sample_gives_the_uniform_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """N = 1, open == close == g: vm_render_halfway's bytes (NaN pixels too: the same conversion in both kernels) and
    vm_render_layers' bits for 1, 3 and 4 channels, every color_from"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    for g in (0.0, 0.3, 1.0):
        for cf in (0, 1, 2):
            out, ref = fr.render_shutter(0.3, g, g, 1, cf), fr.render_halfway(0.3, g, cf)
            assert np.array_equal(out, ref), (g, cf, int((out != ref).sum()))
    for c in (1, 3, 4):
        fr.upload_layers(_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c))
        for g in (0.0, 0.3, 1.0):
            for cf in (0, 1, 2):
                out, ref = fr.render_shutter_layers(0.3, g, g, 1, cf), fr.render_layers(0.3, g, cf)
                assert _same(out, ref), (c, g, cf, int((out != ref).sum()))
    fr.close()


@shapes
@kinds
@cases
def test_shutter_calls_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    """layers of 1, 3 and 4 channels bit for bit, a NaN for a NaN; RGB8 byte for byte wherever every sample's two
    positions are finite; every color_from under one of the shutters"""
    v, u = _field(w, h, kind, with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    lay = {c: (_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)) for c in (1, 3, 4)}
    for n, (o, c) in EVERY:
        maps = _ref_maps(w, h, kind, with_path, o, c, n)
        ok = chain_ref.founded(maps)
        assert kind == "nan" or ok.all()
        cfs = (0, 1, 2) if (n, (o, c)) == EVERY[0] else (1,)
        for cf in cfs:
            got = fr.render_shutter(0.3, o, c, n, cf)
            want = chain_ref.bytes_of(shutter_ref.canvas_mean(e0, e1, ex, maps, 0.3, cf))
            assert np.array_equal(got[ok], want[ok]), (n, o, c, cf, int((got != want)[ok].sum()))
        for ch, (l0, l1) in lay.items():
            fr.upload_layers(l0, l1)
            for cf in cfs:
                got = fr.render_shutter_layers(0.3, o, c, n, cf)
                want = shutter_ref.layers_on_maps(l0, l1, maps, 0.3, cf)
                assert _same(got, want), (ch, n, o, c, cf, int((got != want).sum()))
    fr.close()


@shapes
@cases
def test_a_zero_field_gives_side_0s_image(gpu_ctx, w, h, ex, with_path):
    """every tap lands on a texel: under color_from 0 the output is side 0's image for any shutter and any N (with_path:
    a path of zeros, which takes the kernels that tap u)"""
    v = np.zeros((h, w, 2), f32)
    fr = _frame(gpu_ctx, w, h, ex, v, np.zeros((h, w, 2), f32) if with_path else None)
    rgb0, rgb1 = _rgb(w, h)
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))
    for n in (1, 3, 64):
        for o, c in SHUTTERS:
            assert np.array_equal(fr.render_shutter(0.3, o, c, n, 0), rgb0), (n, o, c)
            assert _same(fr.render_shutter_layers(0.3, o, c, n, 0), rgb0.astype(f32)), (n, o, c)
    fr.close()


@shapes
@pytest.mark.parametrize("kind", ["smooth", "large", "outside"])
@cases
def test_rgb_as_float_layers_rounds_to_the_shutters_bytes(gpu_ctx, w, h, ex, kind, with_path):
    """a frame without an extension whose canvases are the two frames, and the same RGB as 3-channel float layers:
    (uint8)(double(render_shutter_layers) + 0.5) is vm_render_shutter's byte everywhere -- both clamp where a tap leaves
    the image, the renderer's + 0.0f is exact, and the sums and the division are the same float32 operations"""
    fr = _frame(gpu_ctx, w, h, 0, *_field(w, h, kind, with_path))
    rgb0, rgb1 = _rgb(w, h)
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))
    for n, (o, c) in EVERY:
        for cf in ((0, 1, 2) if n == 5 else (1,)):
            lay = fr.render_shutter_layers(0.3, o, c, n, cf)
            assert lay.shape == (h, w, 3) and lay.dtype == np.float32
            out, ref = chain_ref.bytes_of(lay), fr.render_shutter(0.3, o, c, n, cf)
            assert np.array_equal(out, ref), (n, o, c, cf, int((out != ref).sum()))
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from videomorphing_amd import capi, morph, synth
    ctx = morph.Context(0, capi.MATH_FAST)
    for w, h, ex in ((203, 77, 9), (33, 7, 3), (5, 3, 2)):
        rgb0, rgb1 = synth.make_rgb_pair(w, h)
        for kind in ("smooth", "large", "outside", "nan"):
            rng = np.random.RandomState(41)
            v, u = warp_ref.field(kind, w, h, rng), warp_ref.path(w, h, rng)
            fr = morph.Frame(ctx, w, h, ex)
            for path in (None, u):
                hh = hashlib.sha256()
                fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, path)
                for c in (1, 3, 4):
                    fr.upload_layers(np.dstack([rgb0, rgb1]).astype(np.float32)[..., :c] / np.float32(3), np.dstack([rgb1, rgb0]).astype(np.float32)[..., :c])
                    for n, o, cl in ((1, 0.3, 0.3), (2, 0.7, 0.3), (5, 0.0, 1.0), (5, -0.2, 0.2), (16, 0.5, 0.52), (16, 0.3, 0.7)):
                        if c == 1:
                            hh.update(fr.render_shutter(0.3, o, cl, n, 1).tobytes())
                        lay = fr.render_shutter_layers(0.3, o, cl, n, 1)
                        nan = np.isnan(lay)                 # a NaN for a NaN: its sign and payload are not specified
                        hh.update(nan.tobytes())
                        hh.update(np.where(nan, np.float32(0), lay).tobytes())
                print("HASH", w, h, kind, path is not None, hh.hexdigest())
            fr.close()
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain -- also the path of fields of 4 GiB and more) give the window kernels'
    bits, which the tests above hold to the statement: a fresh child process with the switch set hashes, case by case, the
    bytes and the layers of 1, 3 and 4 channels (a NaN for a NaN, bit for bit elsewhere) for every N and every kind of
    shutter, on three shapes and the four fields, with and without a path; another one hashes the window form's"""
    plain, window = hashes_under_render_mode(_PROG, "plain"), hashes_under_render_mode(_PROG, None)
    assert len(window) == 24
    assert plain == window, [a for a, b in zip(plain, window) if a != b]


def test_state_and_errors(gpu_ctx):
    """every error code is the listed one, pitched outputs keep what lies beyond their rows, a positive time, and a frame
    that is what it was after all of it"""
    w, h, ex = 33, 7, 3
    v, u = _field(w, h, "smooth", True)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    L, hnd = fr._L, fr._h
    rgb, out, ms = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 2), f32), C.c_float(-1.0)
    # no layers yet
    assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, 1, out.ctypes.data, 0) == capi.VM_E_STATE
    assert L.vm_render_shutter_layers_dev(hnd, 0.3, 0.4, 0.6, 4, 1, C.byref(ms)) == capi.VM_E_STATE
    with pytest.raises(capi.VmError) as e:
        fr.render_shutter_layers(0.3, 0.4, 0.6, 4)
    assert e.value.code == capi.VM_E_STATE
    fr.render_shutter(0.3, 0.4, 0.6, 4)                 # the canvases need none
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    fr.upload_layers(l0, l1)
    v0, q0, img0, lay0 = fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1)
    for n in (0, -1, 65, 1 << 20):
        assert L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, n, 1, rgb.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_shutter_dev(hnd, 0.3, 0.4, 0.6, n, 1, C.byref(ms)) == capi.VM_E_INVALID
        assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, n, 1, out.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_shutter_layers_dev(hnd, 0.3, 0.4, 0.6, n, 1, C.byref(ms)) == capi.VM_E_INVALID
    for cf in (-1, 3):
        assert L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, 4, cf, rgb.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_shutter_dev(hnd, 0.3, 0.4, 0.6, 4, cf, C.byref(ms)) == capi.VM_E_INVALID
        assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, cf, out.ctypes.data, 0) == capi.VM_E_INVALID
        assert L.vm_render_shutter_layers_dev(hnd, 0.3, 0.4, 0.6, 4, cf, C.byref(ms)) == capi.VM_E_INVALID
    assert L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, 4, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, 4, 1, rgb.ctypes.data, 3 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, 4, 1, rgb.ctypes.data, -1) == capi.VM_E_INVALID
    assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, 1, out.ctypes.data, 2 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, 1, out.ctypes.data, -1) == capi.VM_E_INVALID
    with pytest.raises(capi.VmError) as e:
        fr.render_shutter(0.3, 0.4, 0.6, 65)
    assert e.value.code == capi.VM_E_INVALID
    # 1 and 64 are legal
    fr.render_shutter(0.3, 0.4, 0.6, 64)
    fr.render_shutter_layers(0.3, 0.4, 0.6, 64)
    # pitched outputs keep what lies beyond their rows
    big = np.full((h, 3 * w + 5), 201, np.uint8)
    capi.check(L.vm_render_shutter(hnd, 0.3, 0.4, 0.6, 4, 1, big.ctypes.data, 3 * w + 5))
    assert np.array_equal(big[:, :3 * w].reshape(h, w, 3), fr.render_shutter(0.3, 0.4, 0.6, 4, 1)) and np.all(big[:, 3 * w:] == 201)
    bigf = np.full((h, 2 * w + 3), f32(-12345.5), f32)
    capi.check(L.vm_render_shutter_layers(hnd, 0.3, 0.4, 0.6, 4, 1, bigf.ctypes.data, 2 * w + 3))
    ref = shutter_ref.render_shutter_layers(l0, l1, v, u, 0.3, 0.4, 0.6, 4, 1)
    assert _same(bigf[:, :2 * w].reshape(h, w, 2), ref) and np.all(bigf[:, 2 * w:] == f32(-12345.5))
    assert fr.render_shutter_dev(0.3, 0.4, 0.6, 4) > 0 and fr.render_shutter_layers_dev(0.3, 0.4, 0.6, 4) > 0
    capi.check(L.vm_render_shutter_dev(hnd, 0.3, 0.4, 0.6, 4, 1, None))
    capi.check(L.vm_render_shutter_layers_dev(hnd, 0.3, 0.4, 0.6, 4, 1, None))
    # the frame is what it was
    assert np.array_equal(fr.download_v().view(np.uint32), v0.view(np.uint32))
    assert np.array_equal(fr.download_qpath().view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), img0)
    assert _same(fr.render_layers(0.3, 0.35, 1), lay0)
    fr.close()
