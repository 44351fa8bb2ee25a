"""The kernels of videomorphing_amd/csrc/vm_tshutter.hip behind vm_render_transition_shutter and
vm_render_transition_shutter_layers: tied to the kernels that exist -- one sample at one time gives the transition
kernels' bits, the schedule (0, 1) the shutter kernels' bits, GPU against GPU -- and bit for bit the float32 statement of
tests/transit_shutter_ref.py.

Shapes are those of tests/test_gpu_shutter.py: 203x77 is no multiple of the 32x16 tile, 33x7 one partial tile narrower
than the LDS window (half of its waves have no pixel and are in the loop for the barriers alone), 5x3 smaller than the
window's margin, 138x84 the smoke shape.  Fields: smooth, large, outside and the one with NaN / Inf in it (compared NaN for
NaN, and must not fault).  The schedule is a wipe for the geometry and a radial one for the colour unless said otherwise.

Against the statement: (N, shutter) in (2, (0.7, 0.3)), (5, (0, 1)), (5, (0.50, 0.52)), (3, (-0.2, 0.2)) at t_color = 0.45
with the linear ease, and the second one with the smooth ease: twenty walks of the chain in numpy per case, under two
seconds at 203x77.  Under (0.50, 0.52) the v window does not move while G_s does: a kernel that keeps a stale rate window
differs from the statement on 69 % of the pixels of 203x77 smooth, so this is the case that catches a skipped refill;
under (0, 1) with the large field the window moves about 110 px from sample to sample.  N = 16 runs on 33x7 and 5x3 only,
where a schedule of random pairs with steps among them (t1 <= t0) runs too.  RGB8 bytes are compared where every sample's
two positions are finite (what a NaN becomes as a byte is defined neither by C nor by numpy): everywhere for the three
finite fields, and for the NaN field on a share the test holds to a floor, so that the mask cannot swallow the comparison."""
import ctypes as C
import functools
import os
import textwrap

import numpy as np
import pytest

import chain_ref
import transit_ref
import transit_shutter_ref as TS
from render_cases import field as _field, frame, hashes_under_render_mode, layers as _layers, rgb_pair as _rgb, same_bits as _same
from videomorphing_amd import capi, transition

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SHAPES = [(203, 77, 9), (33, 7, 3), (5, 3, 2), (138, 84, 8)]
SMALL = ((33, 7), (5, 3))
KINDS = ["smooth", "large", "outside", "nan"]
SHUTTERS = ((0.3, 0.7), (0.0, 1.0), (0.50, 0.52), (-0.2, 0.2), (0.7, 0.3))      # tests/test_gpu_shutter.py's five
LINEAR, SMOOTH = capi.EASE_LINEAR, capi.EASE_SMOOTH
# (N, shutter, ease) held to the statement on every shape
STATED = ((2, (0.7, 0.3), LINEAR), (5, (0.0, 1.0), LINEAR), (5, (0.50, 0.52), LINEAR), (3, (-0.2, 0.2), LINEAR),
          (5, (0.0, 1.0), SMOOTH))
T_COLOR = 0.45
# The least share of pixels the NaN field must leave to the RGB8 comparison of a combination.  Under the four linear
# combinations of STATED the statement itself leaves at least 0.31 (203x77, 138x84), 0.08 (19 pixels, 33x7) and one pixel
# (5x3: two with a path); under the smooth one 0.31, 17 pixels -- and none at all at 5x3 without a path, as under some of
# the 16-sample runs there.  So the floor of one pixel is held per combination where `floors` says so and by every case
# as a whole; the two larger shapes hold 0.25 under every combination.
NAN_FLOOR = {(203, 77): 0.25, (33, 7): 1 / (33 * 7), (5, 3): 1 / (5 * 3), (138, 84): 0.25}
cases = pytest.mark.parametrize("with_path", [False, True])
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
kinds = pytest.mark.parametrize("kind", KINDS)


@functools.lru_cache(maxsize=None)
def _schedule(w, h, which):
    """(geometry, colour): the wipe and the radial one, or random pairs with steps (t1 <= t0) among them"""
    if which == "wipe":
        out = transition.wipe(w, h), transition.radial(w, h)
    else:
        rng = np.random.RandomState(97)
        def pairs():
            t0 = rng.uniform(0.0, 0.8, (h, w)).astype(f32)
            return np.stack([t0, t0 + rng.uniform(-0.1, 0.4, (h, w)).astype(f32)], -1)
        out = pairs(), pairs()
        assert (out[0][..., 1] <= out[0][..., 0]).any() and (out[0][..., 1] > out[0][..., 0]).any()
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=256)
def _walk_at(w, h, kind, with_path, which, ease, t_bits):
    """the statement's (map0, map1, k) at one sample time: computed once, shared, never written"""
    sg, sc = _schedule(w, h, which)
    K = transit_ref.ramp(sc, T_COLOR, ease)
    out = TS.walk(*_field(w, h, kind, with_path), transit_ref.ramp(sg, np.uint32(t_bits).view(f32), ease), K)
    for a in out:
        a.setflags(write=False)
    return out


def _ref_maps(w, h, kind, with_path, which, ease, o, c, n):
    return [_walk_at(w, h, kind, with_path, which, ease, int(t.view(np.uint32))) for t in TS.sample_times(o, c, n)]


def _frame(gpu_ctx, w, h, ex, v, u, which="wipe"):
    return frame(gpu_ctx, w, h, ex, v, u, _schedule(w, h, which) if which else None)


@shapes
@kinds
@cases
def test_one_sample_gives_the_transition_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """N = 1, t_open == t_close == t_color == t: vm_render_transition's bytes (NaN pixels too: the same conversion in both
    kernels) and vm_render_transition_layers' bits for 1, 3 and 4 channels, both eases, every color_from"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    every = [(t, e, cf) for t in (0.0, 0.3, 1.0, 1.2) for e in (LINEAR, SMOOTH) for cf in (0, 1, 2)]
    for t, e, cf in every:
        out, ref = fr.render_transition_shutter(t, t, 1, t, e, cf), fr.render_transition(t, e, cf)
        assert np.array_equal(out, ref), (t, e, cf, int((out != ref).sum()))
    for c in (1, 3, 4):
        fr.upload_layers(_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c))
        for t, e, cf in every:
            out, ref = fr.render_transition_shutter_layers(t, t, 1, t, e, cf), fr.render_transition_layers(t, e, cf)
            assert _same(out, ref), (c, t, e, cf, int((out != ref).sum()))
    fr.close()


@shapes
@kinds
@cases
def test_the_uniform_schedule_gives_the_shutter_kernels_bits(gpu_ctx, w, h, ex, kind, with_path):
    """the schedule (0, 1) on both planes, linear ease, t_color = 0.3: vm_render_shutter's bytes and
    vm_render_shutter_layers' bits at color_fa = 0.3 for N in 2, 5, 16 under the five shutters"""
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path), which=None)
    fr.upload_schedule(geo=transition.uniform(w, h), color=None)
    every = [(n, o, c) for n in (2, 5, 16) for o, c in SHUTTERS]
    for n, o, c in every:
        for cf in ((0, 1, 2) if n == 5 else (1,)):
            out, ref = fr.render_transition_shutter(o, c, n, 0.3, LINEAR, cf), fr.render_shutter(0.3, o, c, n, cf)
            assert np.array_equal(out, ref), (n, o, c, cf, int((out != ref).sum()))
    for ch in (1, 3, 4):
        fr.upload_layers(_layers(w, h, ch, 10 + ch), _layers(w, h, ch, 20 + ch))
        for n, o, c in every:
            for cf in ((0, 1, 2) if n == 5 else (1,)):
                out = fr.render_transition_shutter_layers(o, c, n, 0.3, LINEAR, cf)
                ref = fr.render_shutter_layers(0.3, o, c, n, cf)
                assert _same(out, ref), (ch, n, o, c, cf, int((out != ref).sum()))
    fr.close()


def _hold_to_the_statement(fr, w, h, ex, kind, with_path, which, stated, floors):
    """layers of 1, 3 and 4 channels bit for bit at every pixel, a NaN for a NaN; RGB8 byte for byte wherever every
    sample's two positions are finite; every color_from under the first of `stated`.  floors: the combinations of `stated`
    that hold NAN_FLOOR each; the case as a whole holds it in any event."""
    e0, e1 = fr.download_ext(1), fr.download_ext(2)
    lay = {c: (_layers(w, h, c, 10 + c), _layers(w, h, c, 20 + c)) for c in (1, 3, 4)}
    compared = 0
    for n, (o, c), ease in stated:
        maps = _ref_maps(w, h, kind, with_path, which, ease, o, c, n)
        ok = chain_ref.founded(maps)
        share = float(ok.mean())
        compared += int(ok.sum())
        print("founded", w, h, kind, with_path, which, n, o, c, ease, share)
        assert kind == "nan" or ok.all()
        assert (n, (o, c), ease) not in floors or share >= NAN_FLOOR[(w, h)], (n, o, c, ease, share)
        cfs = (0, 1, 2) if (n, (o, c), ease) == stated[0] else (1,)
        for cf in cfs:
            got = fr.render_transition_shutter(o, c, n, T_COLOR, ease, cf)
            want = chain_ref.bytes_of(TS.canvas_mean(e0, e1, ex, maps, cf))
            assert np.array_equal(got[ok], want[ok]), (n, o, c, ease, cf, int((got != want)[ok].sum()), int(ok.sum()))
        for ch, (l0, l1) in lay.items():
            fr.upload_layers(l0, l1)
            for cf in cfs:
                got = fr.render_transition_shutter_layers(o, c, n, T_COLOR, ease, cf)
                want = TS.layers_on_maps(l0, l1, maps, cf)
                assert _same(got, want), (ch, n, o, c, ease, cf, int((got != want).sum()), got.size)
    assert compared >= NAN_FLOOR[(w, h)] * w * h, compared


@shapes
@kinds
@cases
def test_calls_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path):
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path))
    _hold_to_the_statement(fr, w, h, ex, kind, with_path, "wipe", STATED, STATED if (w, h) not in SMALL else STATED[:4])
    fr.close()


@pytest.mark.parametrize("w,h,ex", [s for s in SHAPES if s[:2] in SMALL])
@kinds
@cases
@pytest.mark.parametrize("which", ["wipe", "steps"])
def test_sixteen_samples_and_a_schedule_with_steps_equal_the_statement(gpu_ctx, w, h, ex, kind, with_path, which):
    fr = _frame(gpu_ctx, w, h, ex, *_field(w, h, kind, with_path), which=which)
    stated = ((16, (0.3, 0.7), LINEAR), (16, (0.50, 0.52), SMOOTH))
    if which == "steps":
        stated += STATED[1:4]
    _hold_to_the_statement(fr, w, h, ex, kind, with_path, which, stated, ())
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
            for e in (LINEAR, SMOOTH):
                assert np.array_equal(fr.render_transition_shutter(o, c, n, T_COLOR, e, 0), rgb0), (n, o, c, e)
                assert _same(fr.render_transition_shutter_layers(o, c, n, T_COLOR, e, 0), rgb0.astype(f32)), (n, o, c, e)
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref
    from videomorphing_amd import capi, morph, synth, transition
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
                for c in (1, 3, 4):
                    fr.upload_layers(np.dstack([rgb0, rgb1]).astype(np.float32)[..., :c] / np.float32(3), np.dstack([rgb1, rgb0]).astype(np.float32)[..., :c])
                    for n, o, cl, e in ((1, 0.3, 0.3, 0), (2, 0.7, 0.3, 0), (5, 0.0, 1.0, 1), (5, -0.2, 0.2, 0), (16, 0.5, 0.52, 0), (16, 0.3, 0.7, 1)):
                        if c == 1:
                            hh.update(fr.render_transition_shutter(o, cl, n, 0.45, e, 1).tobytes())
                        lay = fr.render_transition_shutter_layers(o, cl, n, 0.45, e, 1)
                        nan = np.isnan(lay)                 # a NaN for a NaN: its sign and payload are not specified
                        hh.update(nan.tobytes())
                        hh.update(np.where(nan, np.float32(0), lay).tobytes())
                print("HASH", w, h, kind, path is not None, hh.hexdigest())
            fr.close()
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_plain_form_agrees(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain -- also the path of fields of 4 GiB and more) give the window kernels'
    bits, which the tests above hold to the statement: a fresh child process with the switch set hashes, case by case, the
    bytes and the layers of 1, 3 and 4 channels (a NaN for a NaN, bit for bit elsewhere) on three shapes and the four
    fields, with and without a path; another one hashes the window form's"""
    plain, window = hashes_under_render_mode(_PROG, "plain"), hashes_under_render_mode(_PROG, None)
    assert len(window) == 24
    assert plain == window, [a for a, b in zip(plain, window) if a != b]


def test_state_and_errors(gpu_ctx):
    """every error code is the listed one on all four calls, pitched outputs keep what lies beyond their rows, a positive
    time, and a frame that is what it was after all of it"""
    w, h, ex = 33, 7, 3
    v, u = _field(w, h, "smooth", True)
    sg, sc = _schedule(w, h, "wipe")
    fr = _frame(gpu_ctx, w, h, ex, v, u, which=None)
    L, hnd = fr._L, fr._h
    rgb, out, ms = np.zeros((h, w, 3), np.uint8), np.zeros((h, w, 2), f32), C.c_float(-1.0)

    def four(samples=4, ease=LINEAR, cf=1):
        return (L.vm_render_transition_shutter(hnd, 0.4, 0.6, samples, 0.5, ease, cf, rgb.ctypes.data, 0),
                L.vm_render_transition_shutter_dev(hnd, 0.4, 0.6, samples, 0.5, ease, cf, C.byref(ms)),
                L.vm_render_transition_shutter_layers(hnd, 0.4, 0.6, samples, 0.5, ease, cf, out.ctypes.data, 0),
                L.vm_render_transition_shutter_layers_dev(hnd, 0.4, 0.6, samples, 0.5, ease, cf, C.byref(ms)))

    # neither a schedule nor layers; then layers and no schedule
    assert four() == (capi.VM_E_STATE,) * 4
    l0, l1 = _layers(w, h, 2, 1), _layers(w, h, 2, 2)
    fr.upload_layers(l0, l1)
    assert four() == (capi.VM_E_STATE,) * 4
    with pytest.raises(capi.VmError) as e:
        fr.render_transition_shutter(0.4, 0.6, 4)
    assert e.value.code == capi.VM_E_STATE
    fr.close()
    # a schedule and no layers: the canvases need none
    fr = _frame(gpu_ctx, w, h, ex, v, u)
    L, hnd = fr._L, fr._h
    assert four() == (capi.VM_OK, capi.VM_OK, capi.VM_E_STATE, capi.VM_E_STATE)
    with pytest.raises(capi.VmError) as e:
        fr.render_transition_shutter_layers(0.4, 0.6, 4)
    assert e.value.code == capi.VM_E_STATE
    fr.upload_layers(l0, l1)
    before = (fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1),
              fr.render_transition(0.4, SMOOTH, 1)) + fr.transition_maps(0.4, SMOOTH)
    for n in (0, -1, 65, 1 << 20):
        assert four(samples=n) == (capi.VM_E_INVALID,) * 4, n
    for ease in (-1, 2):
        assert four(ease=ease) == (capi.VM_E_INVALID,) * 4, ease
    for cf in (-1, 3):
        assert four(cf=cf) == (capi.VM_E_INVALID,) * 4, cf
    assert L.vm_render_transition_shutter(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_transition_shutter(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, rgb.ctypes.data, 3 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_transition_shutter(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, rgb.ctypes.data, -1) == capi.VM_E_INVALID
    assert L.vm_render_transition_shutter_layers(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_render_transition_shutter_layers(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, out.ctypes.data, 2 * w - 1) == capi.VM_E_INVALID
    assert L.vm_render_transition_shutter_layers(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, out.ctypes.data, -1) == capi.VM_E_INVALID
    with pytest.raises(capi.VmError) as e:
        fr.render_transition_shutter(0.4, 0.6, 65)
    assert e.value.code == capi.VM_E_INVALID
    # 1 and 64 are legal
    assert four(samples=1) == (capi.VM_OK,) * 4 and four(samples=64) == (capi.VM_OK,) * 4
    # the default colour time is the float32 midpoint
    mid = float((f32(0.4) + f32(0.6)) * f32(0.5))
    assert np.array_equal(fr.render_transition_shutter(0.4, 0.6, 4), fr.render_transition_shutter(0.4, 0.6, 4, mid))
    # pitched outputs keep what lies beyond their rows
    big = np.full((h, 3 * w + 5), 201, np.uint8)
    capi.check(L.vm_render_transition_shutter(hnd, 0.4, 0.6, 4, 0.5, SMOOTH, 1, big.ctypes.data, 3 * w + 5))
    assert np.array_equal(big[:, :3 * w].reshape(h, w, 3), fr.render_transition_shutter(0.4, 0.6, 4, 0.5, SMOOTH, 1))
    assert np.all(big[:, 3 * w:] == 201)
    bigf = np.full((h, 2 * w + 3), f32(-12345.5), f32)
    capi.check(L.vm_render_transition_shutter_layers(hnd, 0.4, 0.6, 4, 0.5, SMOOTH, 1, bigf.ctypes.data, 2 * w + 3))
    ref = TS.render_layers(l0, l1, v, u, sg, sc, 0.4, 0.6, 4, 0.5, SMOOTH, 1)
    assert _same(bigf[:, :2 * w].reshape(h, w, 2), ref) and np.all(bigf[:, 2 * w:] == f32(-12345.5))
    assert fr.render_transition_shutter_dev(0.4, 0.6, 4) > 0 and fr.render_transition_shutter_layers_dev(0.4, 0.6, 4) > 0
    capi.check(L.vm_render_transition_shutter_dev(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, None))
    capi.check(L.vm_render_transition_shutter_layers_dev(hnd, 0.4, 0.6, 4, 0.5, LINEAR, 1, None))
    # the frame is what it was
    after = (fr.download_v(), fr.download_qpath(), fr.render_halfway(0.3, 0.35, 1), fr.render_layers(0.3, 0.35, 1),
             fr.render_transition(0.4, SMOOTH, 1)) + fr.transition_maps(0.4, SMOOTH)
    assert len(before) == len(after) == 10
    for k, (a, b) in enumerate(zip(before, after)):
        assert _same(a, b), k
    fr.close()
