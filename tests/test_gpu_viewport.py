"""The viewport kernels (videomorphing_amd/csrc/vm_viewport.hip) behind vm_render_viewport and vm_render_viewport_layers:
tied to the kernels that exist -- the identity viewport gives vm_render_halfway's bytes and vm_render_layers' bits, an
integer crop their slice, a half-size viewport with 2 x 2 samples over a zero field the exact box reduction -- and bit for
bit the float32 statement of tests/viewport_ref.py under zooms, shifts, enlargements, reductions (the plain form), steps
on both sides of 1, overscan, viewports outside the field and outputs smaller than a tile.

Shapes are those of tests/test_gpu_layers.py: 203x77 is no multiple of the 32x16 tile, 33x7 narrower than the LDS window,
5x3 smaller than the window's margin (enlarged tenfold it lies under four tiles), 138x84 the smoke shape.  Fields: smooth,
large, outside and the one with NaN / Inf in it (compared NaN for NaN, and must not fault).  The statement walks the
chain once per sample in numpy, about 6 us per output pixel and sample, so every viewport carries the sample grids its
output can afford -- (1, 1) always, (2, 2) or (3, 2) beside it, (8, 8) on outputs of at most 40 x 24 -- and no case runs
longer than a few seconds.  RGB8 bytes are compared where every sample's two positions are finite: what a NaN becomes as
a byte is defined neither by C nor by numpy."""
import ctypes as C
import os
import textwrap

import numpy as np
import pytest

import chain_ref
import viewport_ref
from render_cases import field as _field, frame as _frame, hashes_under_render_mode, layers as _layers, same_bits as _same
from videomorphing_amd import capi, morph
from videomorphing_amd.viewport import Viewport

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "large", "outside", "nan"]
ABOVE_ONE = float(np.nextafter(f32(1), f32(2)))       # one ulp above 1: the plain form, the window form's bits
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)


def viewports(w, h, ex):
    """{name: (x0, y0, step_x, step_y, out_w, out_h, sample grids)} for a w x h field"""
    vps = {
        "zoom": (10.25, 3.5, 0.4, 0.4, 64, 40, ((1, 1), (3, 2))),                   # 2.5x at a fractional origin, 2 x 3 tiles
        "shift": (0.5, 0.5, 1.0, 1.0, w, h, ((1, 1), (2, 2))),                      # every q half way between texels
        "double": (0.0, 0.0, 0.5, 0.5, 2 * w, 2 * h, ((1, 1), (2, 2)) if w * h < 3000 else ((1, 1),)),
        "half": (0.0, 0.0, 2.0, 2.0, (w + 1) // 2, (h + 1) // 2, ((1, 1), (2, 2), (3, 2))),       # the plain form
        "aniso": (-2.5, 1.25, 0.75, 1.5, w, (h + 1) // 2, ((1, 1), (3, 2))),        # one axis in reach of the window: plain
        "above": (0.0, 0.0, ABOVE_ONE, ABOVE_ONE, min(w, 70), min(h, 40), ((1, 1), (2, 2))),
        "overscan": (-float(ex), -float(ex), 1.0, 1.0, w + 2 * ex, h + 2 * ex, ((1, 1), (2, 2))),
        "outside": (w + 40.0, -h - 30.0, 1.0, 1.0, 40, 24, ((1, 1), (8, 8))),
        "pixel": (w / 3.0, h / 2.0, 0.7, 0.7, 1, 1, ((1, 1), (2, 2), (8, 8))),
        "narrow": (w - 2.75, -1.5, 0.9, 0.3, 5, 24, ((1, 1), (3, 2), (8, 8))),      # narrower than a tile, two tiles high
    }
    if w * h < 100:
        vps["tenfold"] = (0.0, 0.0, 0.1, 0.1, 10 * w, 10 * h, ((1, 1), (2, 2), (3, 2)))       # the whole field under four tiles
    return vps


NAMES = sorted(viewports(203, 77, 9))
EVERY = [(w, h, ex, name) for w, h, ex in SHAPES for name in sorted(viewports(w, h, ex))]


@shapes
@kinds
@cases
def test_the_identity_viewport_gives_the_uniform_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """{0, 0, 1, 1, w, h, 1, 1}: vm_render_halfway's bytes (NaN pixels too: the same conversion in both kernels) and
    vm_render_layers' bits for 1, 3 and 4 channels, every color_from, geo_fa 0, 0.3 and 1; and an integer crop is the slice"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    ident = Viewport.identity(w, h)
    x, y = w // 3, h // 2
    crop = Viewport.crop(x, y, w - x - 1, h - y)
    for g in (0.0, 0.3, 1.0):
        for cf in (0, 1, 2):
            out, ref = fr.render_viewport(ident, 0.3, g, cf), fr.render_halfway(0.3, g, cf)
            assert np.array_equal(out, ref), (g, cf, int((out != ref).sum()))
            out = fr.render_viewport(crop, 0.3, g, cf)
            assert np.array_equal(out, ref[y:, x:w - 1]), (g, cf)
    for c in (1, 3, 4):
        fr.upload_layers(_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c))
        for g in (0.0, 0.3, 1.0):
            for cf in (0, 1, 2):
                out, ref = fr.render_viewport_layers(ident, 0.3, g, cf), fr.render_layers(0.3, g, cf)
                assert _same(out, ref), (c, g, cf, int((out != ref).sum()))
                assert _same(fr.render_viewport_layers(crop, 0.3, g, cf), ref[y:, x:w - 1]), (c, g, cf)
    fr.close()


@pytest.mark.parametrize("w,h,ex,name", EVERY)
@kinds
@cases
def test_viewport_calls_equal_the_statement(gpu_ctx, w, h, ex, name, kind, with_path):
    """RGB8 byte for byte wherever every sample's two positions are finite, layers bit for bit, a NaN for a NaN: every
    color_from under the first sample grid, 1..4 channels in turn over the viewports (all of them under the first three)"""
    v, u = _field(w, h, kind, with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    x0, y0, sx, sy, ow, oh, grids = viewports(w, h, ex)[name]
    at = NAMES.index(name) if name in NAMES else 0
    chans = (1, 2, 3, 4) if at < 3 else ((at % 4) + 1,)
    lay = {c: (_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)) for c in chans}
    for k, (nx, ny) in enumerate(grids):
        vp = Viewport(x0, y0, sx, sy, ow, oh, nx, ny).validate()
        maps = viewport_ref.sample_maps(v, u, 0.3, vp.astuple())
        ok = chain_ref.founded(maps)
        assert kind == "nan" or ok.all()
        cfs = (0, 1, 2) if k == 0 else (1,)
        for cf in cfs:
            got = fr.render_viewport(vp, 0.3, 0.3, cf)
            want = viewport_ref.render_viewport_bytes(e0, e1, ex, v, u, 0.3, 0.3, cf, vp.astuple(), maps)
            assert got.shape == (oh, ow, 3) and np.array_equal(got[ok], want[ok]), (nx, ny, cf, int((got != want)[ok].sum()))
        for ch, (l0, l1) in lay.items():
            fr.upload_layers(l0, l1)
            for cf in cfs:
                got = fr.render_viewport_layers(vp, 0.3, 0.3, cf)
                want = viewport_ref.layers_on_maps(l0, l1, maps, 0.3, cf)
                assert _same(got, want), (ch, nx, ny, cf, int((got != want).sum()))
    fr.close()


@cases
def test_half_size_with_2x2_samples_is_the_exact_box(gpu_ctx, with_path):
    """zero field (with_path: a path of zeros, which keeps the taps of u), {0, 0, 2, 2, w / 2, h / 2, 2, 2}: every sample
    lands on a texel, the result is (uint8)(sum / 4 + 0.5) of each 2 x 2 block of a random canvas"""
    w, h, ex = 138, 84, 8
    rng = np.random.RandomState(3)
    rgb = [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for _ in range(2)]
    fr = morph.Frame(gpu_ctx, w, h, ex)
    zero = np.zeros((h, w, 2), f32)
    fr.upload(morph.make_extended(rgb[0], ex), morph.make_extended(rgb[1], ex), zero, zero if with_path else None)
    vp = Viewport.fit(w, h, w // 2, h // 2).supersampled(2)
    for cf, src in ((0, rgb[0]), (2, rgb[1])):
        s = src.astype(np.int64)
        box = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
        assert np.array_equal(fr.render_viewport(vp, 0.3, 0.35, cf), (box / 4.0 + 0.5).astype(np.uint8)), cf
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from test_gpu_viewport import viewports
    from videomorphing_amd import capi, morph, synth
    from videomorphing_amd.viewport import Viewport
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
                    for name, (x0, y0, sx, sy, ow, oh, grids) in sorted(viewports(w, h, ex).items()):
                        for nx, ny in grids:
                            vp = Viewport(x0, y0, sx, sy, ow, oh, nx, ny)
                            if c == 1:
                                hh.update(fr.render_viewport(vp, 0.3, 0.3, 1).tobytes())
                            lay = fr.render_viewport_layers(vp, 0.3, 0.3, 1)
                            nan = np.isnan(lay)                 # a NaN for a NaN: its sign and payload are not specified
                            hh.update(nan.tobytes())
                            hh.update(np.where(nan, np.float32(0), lay).tobytes())
                print("HASH", w, h, kind, path is not None, hh.hexdigest())
            fr.close()
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain -- also the path of fields of 4 GiB and more, and of steps above 1) give
    the window kernels' bits, which the tests above hold to the statement: a fresh child process with the switch set
    hashes, case by case, the bytes and the layers of 1, 3 and 4 channels (a NaN for a NaN, bit for bit elsewhere) under
    every viewport and sample grid of this file, on three shapes and the four fields, with and without a path; another
    one hashes the window form's"""
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
    good = Viewport(2.25, 0.5, 0.8, 0.8, 21, 6, 2, 2)
    ow, oh = good.out_w, good.out_h
    gs = good.struct()
    rgb, out, ms = np.zeros((oh, ow, 3), np.uint8), np.zeros((oh, ow, 2), f32), C.c_float(-1.0)
    # no layers yet
    assert L.vm_render_viewport_layers(hnd, C.byref(gs), 0.3, 0.3, 1, out.ctypes.data, 0) == capi.VM_E_STATE
    assert L.vm_render_viewport_layers_dev(hnd, C.byref(gs), 0.3, 0.3, 1, C.byref(ms)) == capi.VM_E_STATE
    with pytest.raises(capi.VmError) as e:
        fr.render_viewport_layers(good, 0.3, 0.3)
    assert e.value.code == capi.VM_E_STATE
    fr.render_viewport(good, 0.3, 0.3)                  # the canvases need none
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    fr.upload_layers(l0, l1)
    v0, q0, img0, lay0 = fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1)
    big_rgb, big_out = np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 2), f32)

    def all_four(s, cf=1):
        p = C.byref(s) if s is not None else None
        return (L.vm_render_viewport(hnd, p, 0.3, 0.3, cf, big_rgb.ctypes.data, 0),
                L.vm_render_viewport_dev(hnd, p, 0.3, 0.3, cf, C.byref(ms)),
                L.vm_render_viewport_layers(hnd, p, 0.3, 0.3, cf, big_out.ctypes.data, 0),
                L.vm_render_viewport_layers_dev(hnd, p, 0.3, 0.3, cf, C.byref(ms)))

    for bad in viewport_ref.INVALID_VIEWPORTS:
        assert all_four(Viewport(*bad).struct()) == (capi.VM_E_INVALID,) * 4, bad
        with pytest.raises(ValueError):
            Viewport(*bad).validate()
        with pytest.raises(capi.VmError) as e:
            fr.render_viewport(Viewport(*bad), 0.3, 0.3)
        assert e.value.code == capi.VM_E_INVALID
    assert all_four(None) == (capi.VM_E_INVALID,) * 4
    for cf in (-1, 3):
        assert all_four(gs, cf) == (capi.VM_E_INVALID,) * 4
    assert L.vm_render_viewport(hnd, C.byref(gs), 0.3, 0.3, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_viewport(hnd, C.byref(gs), 0.3, 0.3, 1, rgb.ctypes.data, 3 * ow - 1) == capi.VM_E_INVALID
    assert L.vm_render_viewport(hnd, C.byref(gs), 0.3, 0.3, 1, rgb.ctypes.data, -1) == capi.VM_E_INVALID
    assert L.vm_render_viewport_layers(hnd, C.byref(gs), 0.3, 0.3, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_viewport_layers(hnd, C.byref(gs), 0.3, 0.3, 1, out.ctypes.data, 2 * ow - 1) == capi.VM_E_INVALID
    assert L.vm_render_viewport_layers(hnd, C.byref(gs), 0.3, 0.3, 1, out.ctypes.data, -1) == capi.VM_E_INVALID
    # the edges are legal (the second one's corner is a million pixels away: the chain clamps as it does for any warp)
    for edge in viewport_ref.EDGE_VIEWPORTS:
        assert fr.render_viewport(Viewport(*edge), 0.3, 0.3).shape == (edge[5], edge[4], 3)
        assert fr.render_viewport_layers(Viewport(*edge), 0.3, 0.3).shape == (edge[5], edge[4], 2)
    # pitched outputs keep what lies beyond their rows
    big = np.full((oh, 3 * ow + 5), 201, np.uint8)
    capi.check(L.vm_render_viewport(hnd, C.byref(gs), 0.3, 0.3, 1, big.ctypes.data, 3 * ow + 5))
    assert np.array_equal(big[:, :3 * ow].reshape(oh, ow, 3), fr.render_viewport(good, 0.3, 0.3, 1)) and np.all(big[:, 3 * ow:] == 201)
    bigf = np.full((oh, 2 * ow + 3), f32(-12345.5), f32)
    capi.check(L.vm_render_viewport_layers(hnd, C.byref(gs), 0.3, 0.3, 1, bigf.ctypes.data, 2 * ow + 3))
    ref = viewport_ref.render_viewport_layers(l0, l1, v, u, 0.3, 0.3, 1, good.astuple())
    assert _same(bigf[:, :2 * ow].reshape(oh, ow, 2), ref) and np.all(bigf[:, 2 * ow:] == f32(-12345.5))
    assert fr.render_viewport_dev(good, 0.3, 0.3) > 0 and fr.render_viewport_layers_dev(good, 0.3, 0.3) > 0
    capi.check(L.vm_render_viewport_dev(hnd, C.byref(gs), 0.3, 0.3, 1, None))
    capi.check(L.vm_render_viewport_layers_dev(hnd, C.byref(gs), 0.3, 0.3, 1, None))
    # the frame is what it was
    assert np.array_equal(fr.download_v().view(np.uint32), v0.view(np.uint32))
    assert np.array_equal(fr.download_qpath().view(np.uint32), q0.view(np.uint32))
    assert np.array_equal(fr.render_halfway(0.3, 0.35, 1), img0)
    assert _same(fr.render_layers(0.3, 0.35, 1), lay0)
    fr.close()
