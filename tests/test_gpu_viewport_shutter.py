"""The kernels of videomorphing_amd/csrc/vm_vshutter.hip behind vm_render_viewport_shutter[_layers] and
vm_render_viewport_transition_shutter[_layers]: bit for bit the float32 statement of tests/vshutter_ref.py, tied GPU
against GPU to the kernels that exist (one time sample: the viewport kernels; the identity viewport: the two shutters'
kernels and, with one sample, the transition kernels; the schedule (0, 1): the uniform family), the plain form against
the window form, and the calls' state and errors.

Shapes and fields are those of tests/test_gpu_viewport.py, the viewports eight of its table.  203x77 is no multiple of the
32x16 tile; 5x3 and the `narrow` and `pixel` viewports leave threads of a workgroup without a pixel, which stay in both
loops for the barriers alone; under the `large` field the window's origin moves from one time sample to the next, under
(0.50, 0.52) it stays while G changes; `half`, `aniso` and `above` run the plain form.  The statement walks the chain once
per time sample and sub-sample in numpy, about 6 us per output pixel and chain, so every viewport carries the
combinations (T, grid, shutter) its output can afford (COMBOS) and no case runs longer than a few seconds.  RGB8 bytes
are compared where every sample's two positions are finite (what a NaN becomes as a byte is defined neither by C nor by
numpy): everywhere for the three finite fields, which the test asserts."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

import chain_ref
import transit_ref
import viewport_ref
import vshutter_ref as VS
from render_cases import field as _field, frame, hashes_under_render_mode, layers as _layers, same_bits as _same
from test_gpu_viewport import viewports
from videomorphing_amd import capi, morph, transition
from videomorphing_amd.viewport import Viewport

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
KINDS = ["smooth", "large", "outside", "nan"]
NAMES = ["zoom", "shift", "overscan", "narrow", "pixel", "half", "aniso", "above"]
LINEAR, SMOOTH = capi.EASE_LINEAR, capi.EASE_SMOOTH
SHUTTERS = ((0.3, 0.7), (0.0, 1.0), (0.50, 0.52), (-0.2, 0.2), (0.8, 1.2), (0.7, 0.3))
COLOR_FA, T_COLOR = 0.3, 0.45
# (T, (nx, ny), (open, close)) per viewport: open > close, a shutter across t = 0 and across t = 1, the whole morph and a
# short exposure, T in 1, 2, 5, 16 and the grids (1, 1), (2, 2), (3, 2) spread over them; (8, 8) at T = 4 is the cap exactly
COMBOS = {
    "zoom": ((2, (2, 2), (0.7, 0.3)), (5, (3, 2), (0.0, 1.0)), (16, (1, 1), (-0.2, 0.2))),
    "shift": ((2, (2, 2), (0.8, 1.2)), (5, (1, 1), (0.0, 1.0))),
    "overscan": ((2, (1, 1), (0.7, 0.3)), (1, (2, 2), (0.3, 0.3))),
    "narrow": ((16, (3, 2), (0.0, 1.0)), (4, (8, 8), (0.7, 0.3)), (5, (1, 1), (0.50, 0.52)), (2, (2, 2), (-0.2, 0.2))),
    "pixel": ((16, (2, 2), (0.0, 1.0)), (4, (8, 8), (0.8, 1.2)), (5, (3, 2), (0.50, 0.52)), (1, (1, 1), (0.3, 0.3))),
    "half": ((2, (2, 2), (0.7, 0.3)), (5, (1, 1), (0.0, 1.0)), (16, (1, 1), (0.8, 1.2)), (1, (3, 2), (0.3, 0.3))),
    "aniso": ((2, (3, 2), (-0.2, 0.2)), (5, (1, 1), (0.0, 1.0))),
    "above": ((2, (2, 2), (0.0, 1.0)), (5, (3, 2), (0.50, 0.52)), (16, (1, 1), (0.7, 0.3))),
}
SCHEDULES = ("wipe", "halves", "radial")
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)
names = pytest.mark.parametrize("name", NAMES)


@functools.lru_cache(maxsize=None)
def _schedule(w, h, which):
    """(geometry, colour) of the transition tests: a wipe with a radial colour, two halves, a radial one with a wipe"""
    out = {"wipe": lambda: (transition.wipe(w, h), transition.radial(w, h)),
           "halves": lambda: (transit_ref.two_halves(w, h), transition.radial(w, h)),
           "radial": lambda: (transition.radial(w, h), transition.wipe(w, h))}[which]()
    out = tuple(np.ascontiguousarray(a, dtype=f32) for a in out)
    for a in out:
        a.setflags(write=False)
    return out


def _frame(gpu_ctx, w, h, ex, v, u, which=None):
    return frame(gpu_ctx, w, h, ex, v, u, _schedule(w, h, which) if which else None)


def _viewport(w, h, ex, name, grid):
    x0, y0, sx, sy, ow, oh, _ = viewports(w, h, ex)[name]
    return Viewport(x0, y0, sx, sy, ow, oh, *grid).validate()


def stated(w, h, ex, name, kind, with_path):
    """[(family, T, vp, (open, close), ease, maps)] of a case: the statement's sample maps of both families under every
    combination of the viewport; the scheduled family's ease alternates, its schedule goes by the viewport"""
    v, u = _field(w, h, kind, with_path)
    which = SCHEDULES[NAMES.index(name) % 3]
    sg, sc = _schedule(w, h, which)
    out = []
    for k, (n, grid, (o, c)) in enumerate(COMBOS[name]):
        vp = _viewport(w, h, ex, name, grid)
        out.append(("uniform", n, vp, (o, c), None, VS.uniform_maps(v, u, o, c, n, vp.astuple())))
        ease = (LINEAR, SMOOTH)[k % 2]
        out.append(("scheduled", n, vp, (o, c), ease, VS.scheduled_maps(v, u, sg, sc, o, c, n, T_COLOR, ease, vp.astuple())))
    return which, out


@shapes
@names
@kinds
@cases
def test_calls_equal_the_statement(gpu_ctx, w, h, ex, name, kind, with_path):
    """RGB8 byte for byte wherever every sample's two positions are finite -- everywhere but under the NaN field --,
    layers bit for bit, a NaN for a NaN: every color_from under the first combination, 1..4 channels in turn over the
    viewports (all of them under the first two)"""
    v, u = _field(w, h, kind, with_path)
    which, every = stated(w, h, ex, name, kind, with_path)
    fr = _frame(gpu_ctx, w, h, ex, v, u, which)
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    at = NAMES.index(name)
    chans = (1, 2, 3, 4) if at < 2 else ((at % 4) + 1,)
    lay = {c: (_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)) for c in chans}
    for k, (family, n, vp, (o, c), ease, maps) in enumerate(every):
        ok = chain_ref.founded(maps)
        print("founded", w, h, name, kind, with_path, family, n, (vp.nx, vp.ny), o, c, float(ok.mean()))
        assert kind == "nan" or ok.all(), (family, n, o, c)
        cfs = (0, 1, 2) if k < 2 else (1,)
        uniform = family == "uniform"
        for cf in cfs:
            if uniform:
                got = fr.render_viewport_shutter(vp, COLOR_FA, o, c, n, cf)
                want = VS.bytes_on_maps(e0, e1, ex, maps, cf, COLOR_FA)
            else:
                got = fr.render_viewport_transition_shutter(vp, o, c, n, T_COLOR, ease, cf)
                want = VS.bytes_on_maps(e0, e1, ex, maps, cf)
            assert got.shape == (vp.out_h, vp.out_w, 3)
            assert np.array_equal(got[ok], want[ok]), (family, n, vp, o, c, ease, cf, int((got != want)[ok].sum()), int(ok.sum()))
        for ch, (l0, l1) in lay.items():
            fr.upload_layers(l0, l1)
            for cf in cfs:
                if uniform:
                    got = fr.render_viewport_shutter_layers(vp, COLOR_FA, o, c, n, cf)
                    want = VS.layers_on_maps(l0, l1, maps, cf, COLOR_FA)
                else:
                    got = fr.render_viewport_transition_shutter_layers(vp, o, c, n, T_COLOR, ease, cf)
                    want = VS.layers_on_maps(l0, l1, maps, cf)
                assert _same(got, want), (family, ch, n, vp, o, c, ease, cf, int((got != want).sum()), got.size)
    fr.close()


def _tie_viewports(w, h, ex):
    return [_viewport(w, h, ex, "zoom", (3, 2)), _viewport(w, h, ex, "narrow", (8, 8)), _viewport(w, h, ex, "pixel", (2, 2)),
            _viewport(w, h, ex, "half", (2, 2)), _viewport(w, h, ex, "overscan", (1, 1))]


@shapes
@kinds
@cases
def test_one_time_sample_gives_the_viewport_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """T = 1, open == close == g in 0, 0.3, 1: vm_render_viewport's bytes (NaN pixels too: the same conversion in both
    kernels) and vm_render_viewport_layers' bits for 1, 3 and 4 channels, every color_from"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    vps = _tie_viewports(w, h, ex)
    every = [(vp, g, cf) for vp in vps for g in (0.0, 0.3, 1.0) for cf in (0, 1, 2)]
    for vp, g, cf in every:
        out, ref = fr.render_viewport_shutter(vp, COLOR_FA, g, g, 1, cf), fr.render_viewport(vp, COLOR_FA, g, cf)
        assert np.array_equal(out, ref), (vp, g, cf, int((out != ref).sum()))
    for ch in (1, 3, 4):
        fr.upload_layers(_layers(w, h, ch, 10 + ch), _layers(w, h, ch, 20 + ch))
        for vp, g, cf in every:
            out, ref = fr.render_viewport_shutter_layers(vp, COLOR_FA, g, g, 1, cf), fr.render_viewport_layers(vp, COLOR_FA, g, cf)
            assert _same(out, ref), (ch, vp, g, cf, int((out != ref).sum()))
    fr.close()


@shapes
@kinds
@cases
def test_the_identity_viewport_gives_the_shutter_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """{0, 0, 1, 1, w, h, 1, 1}: vm_render_shutter[_layers]' bits for T in 1, 2, 5, 16 under the six shutters; under the
    schedule vm_render_transition_shutter[_layers]' with both eases, and with one sample at one time
    vm_render_transition[_layers]'; and through the facade render_viewport_transition"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path), which="wipe")
    ident = Viewport.identity(w, h)
    every = [(n, o, c) for n in (1, 2, 5, 16) for o, c in SHUTTERS]
    instants = [(t, e) for t in (0.0, 0.3, 1.0, 1.2) for e in (LINEAR, SMOOTH)]

    def both(layers):
        sh = fr.render_viewport_shutter_layers if layers else fr.render_viewport_shutter
        sh0 = fr.render_shutter_layers if layers else fr.render_shutter
        ts = fr.render_viewport_transition_shutter_layers if layers else fr.render_viewport_transition_shutter
        ts0 = fr.render_transition_shutter_layers if layers else fr.render_transition_shutter
        tr0 = fr.render_transition_layers if layers else fr.render_transition
        for n, o, c in every:
            for cf in ((0, 1, 2) if n == 5 else (1,)):
                out, ref = sh(ident, COLOR_FA, o, c, n, cf), sh0(COLOR_FA, o, c, n, cf)
                assert _same(out, ref), (layers, n, o, c, cf, int((out != ref).sum()))
                for e in (LINEAR, SMOOTH):
                    out, ref = ts(ident, o, c, n, T_COLOR, e, cf), ts0(o, c, n, T_COLOR, e, cf)
                    assert _same(out, ref), (layers, n, o, c, e, cf, int((out != ref).sum()))
        for t, e in instants:
            for cf in (0, 1, 2):
                out, ref = ts(ident, t, t, 1, t, e, cf), tr0(t, e, cf)
                assert _same(out, ref), (layers, t, e, cf, int((out != ref).sum()))

    both(False)
    for t, e in instants:
        assert np.array_equal(fr.render_viewport_transition(ident, t, e, 1), fr.render_transition(t, e, 1)), (t, e)
    for ch in (1, 3, 4):
        fr.upload_layers(_layers(w, h, ch, 10 + ch), _layers(w, h, ch, 20 + ch))
        both(True)
    fr.close()


@shapes
@kinds
@cases
def test_the_uniform_schedule_gives_the_uniform_familys_bits(gpu_ctx, w, h, ex, kind, with_path):
    """the schedule (0, 1) on both planes, linear ease: the uniform family's bytes and bits at color_fa = t_color in
    0, 0.3, 1, through viewports of both forms"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    fr.upload_schedule(geo=transition.uniform(w, h), color=None)
    vps = _tie_viewports(w, h, ex)[:4]
    every = [(vp, n, o, c) for vp in vps for (n, (o, c)) in zip((2, 5, 16, 1, 4, 3), SHUTTERS) if n * vp.nx * vp.ny <= 256]
    for vp, n, o, c in every:
        for tc in (0.0, 0.3, 1.0):
            for cf in ((0, 1, 2) if n == 5 else (1,)):
                out = fr.render_viewport_transition_shutter(vp, o, c, n, tc, LINEAR, cf)
                ref = fr.render_viewport_shutter(vp, tc, o, c, n, cf)
                assert np.array_equal(out, ref), (vp, n, o, c, tc, cf, int((out != ref).sum()))
    for ch in (1, 3, 4):
        fr.upload_layers(_layers(w, h, ch, 10 + ch), _layers(w, h, ch, 20 + ch))
        for vp, n, o, c in every:
            for cf in ((0, 1, 2) if n == 5 else (1,)):
                out = fr.render_viewport_transition_shutter_layers(vp, o, c, n, 0.3, LINEAR, cf)
                ref = fr.render_viewport_shutter_layers(vp, 0.3, o, c, n, cf)
                assert _same(out, ref), (ch, vp, n, o, c, cf, int((out != ref).sum()))
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from test_gpu_viewport import viewports
    from test_gpu_viewport_shutter import COMBOS, NAMES
    from videomorphing_amd import capi, morph, synth, transition
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
                fr.upload_schedule(transition.wipe(w, h), transition.radial(w, h))
                def take(rgb, lay):
                    if rgb is not None:
                        hh.update(rgb.tobytes())
                    nan = np.isnan(lay)                 # a NaN for a NaN: its sign and payload are not specified
                    hh.update(nan.tobytes())
                    hh.update(np.where(nan, np.float32(0), lay).tobytes())
                for c in (1, 3, 4):
                    fr.upload_layers(np.dstack([rgb0, rgb1]).astype(np.float32)[..., :c] / np.float32(3), np.dstack([rgb1, rgb0]).astype(np.float32)[..., :c])
                    for name in NAMES:
                        x0, y0, sx, sy, ow, oh, _ = viewports(w, h, ex)[name]
                        for k, (n, (nx, ny), (o, cl)) in enumerate(COMBOS[name]):
                            vp = Viewport(x0, y0, sx, sy, ow, oh, nx, ny)
                            take(fr.render_viewport_shutter(vp, 0.3, o, cl, n, 1) if c == 1 else None,
                                 fr.render_viewport_shutter_layers(vp, 0.3, o, cl, n, 1))
                            take(fr.render_viewport_transition_shutter(vp, o, cl, n, 0.45, k %% 2, 1) if c == 1 else None,
                                 fr.render_viewport_transition_shutter_layers(vp, o, cl, n, 0.45, k %% 2, 1))
                print("HASH", w, h, kind, path is not None, hh.hexdigest())
            fr.close()
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain -- also the path of fields of 4 GiB and more, and of steps above 1) give
    the window kernels' bits, which the tests above hold to the statement: a fresh child process with the switch set
    hashes, case by case, the bytes and the layers of 1, 3 and 4 channels (a NaN for a NaN, bit for bit elsewhere) of both
    families under every viewport and combination of this file, on three shapes and the four fields, with and without a
    path; another one hashes the window form's"""
    plain, window = hashes_under_render_mode(_PROG, "plain"), hashes_under_render_mode(_PROG, None)
    assert len(window) == 24
    assert plain == window, [a for a, b in zip(plain, window) if a != b]


def test_state_and_errors(gpu_ctx):
    """every error code is the listed one on all eight calls, the cap of 256 chains on both sides, pitched outputs keep
    what lies beyond their rows, a positive time, and a frame that is what it was after all of it"""
    w, h, ex = 33, 7, 3
    v, u = _field(w, h, "smooth", True)
    sg, sc = _schedule(w, h, "wipe")
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    L, hnd = fr._L, fr._h
    good = Viewport(2.25, 0.5, 0.8, 0.8, 21, 6, 2, 2)
    ow, oh = good.out_w, good.out_h
    gs = good.struct()
    ms = C.c_float(-1.0)
    big_rgb, big_out = np.zeros((64, 64, 3), np.uint8), np.zeros((64, 64, 2), f32)

    def eight(s=gs, samples=4, ease=LINEAR, cf=1):
        p = C.byref(s) if s is not None else None
        return (L.vm_render_viewport_shutter(hnd, p, 0.3, 0.4, 0.6, samples, cf, big_rgb.ctypes.data, 0),
                L.vm_render_viewport_shutter_dev(hnd, p, 0.3, 0.4, 0.6, samples, cf, C.byref(ms)),
                L.vm_render_viewport_shutter_layers(hnd, p, 0.3, 0.4, 0.6, samples, cf, big_out.ctypes.data, 0),
                L.vm_render_viewport_shutter_layers_dev(hnd, p, 0.3, 0.4, 0.6, samples, cf, C.byref(ms)),
                L.vm_render_viewport_transition_shutter(hnd, p, 0.4, 0.6, samples, 0.5, ease, cf, big_rgb.ctypes.data, 0),
                L.vm_render_viewport_transition_shutter_dev(hnd, p, 0.4, 0.6, samples, 0.5, ease, cf, C.byref(ms)),
                L.vm_render_viewport_transition_shutter_layers(hnd, p, 0.4, 0.6, samples, 0.5, ease, cf, big_out.ctypes.data, 0),
                L.vm_render_viewport_transition_shutter_layers_dev(hnd, p, 0.4, 0.6, samples, 0.5, ease, cf, C.byref(ms)))

    OK, ST, INV = capi.VM_OK, capi.VM_E_STATE, capi.VM_E_INVALID
    # neither a schedule nor layers; then layers and no schedule; then both
    assert eight() == (OK, OK, ST, ST, ST, ST, ST, ST)
    with pytest.raises(capi.VmError) as e:
        fr.render_viewport_shutter_layers(good, 0.3, 0.4, 0.6, 4)
    assert e.value.code == ST
    with pytest.raises(capi.VmError) as e:
        fr.render_viewport_transition(good, 0.4)
    assert e.value.code == ST
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    fr.upload_layers(l0, l1)
    assert eight() == (OK, OK, OK, OK, ST, ST, ST, ST)
    fr.close()
    fr = _frame(gpu_ctx, w, h, ex, v, u, "wipe")
    L, hnd = fr._L, fr._h
    assert eight() == (OK, OK, ST, ST, OK, OK, ST, ST)
    fr.upload_layers(l0, l1)
    assert eight() == (OK,) * 8
    before = (fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1),
              fr.render_transition(0.4, SMOOTH, 1)) + fr.transition_maps(0.4, SMOOTH)
    # what the viewport section refuses
    for bad in viewport_ref.INVALID_VIEWPORTS:
        assert eight(Viewport(*bad).struct()) == (INV,) * 8, bad
        with pytest.raises(capi.VmError) as e:
            fr.render_viewport_shutter(Viewport(*bad), 0.3, 0.4, 0.6, 4)
        assert e.value.code == INV
    assert eight(None) == (INV,) * 8
    # what the shutter sections refuse (the ease is the scheduled family's alone)
    for n in (0, -1, 65, 1 << 20):
        assert eight(samples=n) == (INV,) * 8, n
    for ease in (-1, 2):
        assert eight(ease=ease) == (OK,) * 4 + (INV,) * 4, ease
    for cf in (-1, 3):
        assert eight(cf=cf) == (INV,) * 8, cf
    # the cap: samples * nx * ny <= 256 -- 4 * 8 * 8 is taken, 5 * 8 * 8 is not, nor 64 * 3 * 2; 64 * 2 * 2 is
    cap = Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 8, 8).struct()
    assert eight(cap, samples=4) == (OK,) * 8 and eight(cap, samples=5) == (INV,) * 8
    assert eight(Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 3, 2).struct(), samples=64) == (INV,) * 8
    assert eight(Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 2, 2).struct(), samples=64) == (OK,) * 8
    assert eight(Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 1, 1).struct(), samples=64) == (OK,) * 8
    Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 8, 8).validate()                # the viewport alone is a good one
    with pytest.raises(capi.VmError) as e:
        fr.render_viewport_transition_shutter(Viewport(0.5, 0.5, 1.0, 1.0, 2, 2, 8, 8), 0.4, 0.6, 5)
    assert e.value.code == INV
    # NULL outputs and pitches below the row
    rgb, out = np.zeros((oh, ow, 3), np.uint8), np.zeros((oh, ow, 2), f32)
    p = C.byref(gs)
    for data, pitch in ((None, 0), (rgb.ctypes.data, 3 * ow - 1), (rgb.ctypes.data, -1)):
        assert L.vm_render_viewport_shutter(hnd, p, 0.3, 0.4, 0.6, 4, 1, data, pitch) == INV
        assert L.vm_render_viewport_transition_shutter(hnd, p, 0.4, 0.6, 4, 0.5, LINEAR, 1, data, pitch) == INV
    for data, pitch in ((None, 0), (out.ctypes.data, 2 * ow - 1), (out.ctypes.data, -1)):
        assert L.vm_render_viewport_shutter_layers(hnd, p, 0.3, 0.4, 0.6, 4, 1, data, pitch) == INV
        assert L.vm_render_viewport_transition_shutter_layers(hnd, p, 0.4, 0.6, 4, 0.5, LINEAR, 1, data, pitch) == INV
    # the edges of the viewport section are legal
    for edge in viewport_ref.EDGE_VIEWPORTS:
        n = 256 // (edge[6] * edge[7])
        assert fr.render_viewport_shutter(Viewport(*edge), 0.3, 0.4, 0.6, min(n, 64)).shape == (edge[5], edge[4], 3)
        assert fr.render_viewport_transition_shutter_layers(Viewport(*edge), 0.4, 0.6, min(n, 64)).shape == (edge[5], edge[4], 2)
    # the default colour time is the float32 midpoint
    mid = float((f32(0.4) + f32(0.6)) * f32(0.5))
    assert np.array_equal(fr.render_viewport_transition_shutter(good, 0.4, 0.6, 4), fr.render_viewport_transition_shutter(good, 0.4, 0.6, 4, mid))
    # pitched outputs keep what lies beyond their rows
    big = np.full((oh, 3 * ow + 5), 201, np.uint8)
    capi.check(L.vm_render_viewport_shutter(hnd, p, 0.3, 0.4, 0.6, 4, 1, big.ctypes.data, 3 * ow + 5))
    assert np.array_equal(big[:, :3 * ow].reshape(oh, ow, 3), fr.render_viewport_shutter(good, 0.3, 0.4, 0.6, 4, 1))
    assert np.all(big[:, 3 * ow:] == 201)
    bigf = np.full((oh, 2 * ow + 3), f32(-12345.5), f32)
    capi.check(L.vm_render_viewport_transition_shutter_layers(hnd, p, 0.4, 0.6, 4, 0.5, SMOOTH, 1, bigf.ctypes.data, 2 * ow + 3))
    ref = VS.render_viewport_transition_shutter_layers(l0, l1, v, u, sg, sc, 0.4, 0.6, 4, 0.5, SMOOTH, 1, good.astuple())
    assert _same(bigf[:, :2 * ow].reshape(oh, ow, 2), ref) and np.all(bigf[:, 2 * ow:] == f32(-12345.5))
    assert fr.render_viewport_shutter_dev(good, 0.3, 0.4, 0.6, 4) > 0 and fr.render_viewport_shutter_layers_dev(good, 0.3, 0.4, 0.6, 4) > 0
    assert fr.render_viewport_transition_shutter_dev(good, 0.4, 0.6, 4) > 0
    assert fr.render_viewport_transition_shutter_layers_dev(good, 0.4, 0.6, 4) > 0
    capi.check(L.vm_render_viewport_shutter_dev(hnd, p, 0.3, 0.4, 0.6, 4, 1, None))
    capi.check(L.vm_render_viewport_transition_shutter_layers_dev(hnd, p, 0.4, 0.6, 4, 0.5, LINEAR, 1, None))
    # the frame is what it was: v, path, canvases, layers and schedule, and an existing uniform render gives the same bytes
    after = (fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1),
             fr.render_transition(0.4, SMOOTH, 1)) + fr.transition_maps(0.4, SMOOTH)
    assert len(before) == len(after) == 10
    for k, (a, b) in enumerate(zip(before, after)):
        assert _same(a, b), k
    fr.close()
