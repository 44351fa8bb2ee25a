"""The multiband kernels (videomorphing_amd/csrc/vm_multiband.hip) behind vm_frame_render_multiband[_layers] and their
transition forms, held to the float32 statement of tests/multiband_ref.py: whole calls byte for byte (RGB8) and bit for bit
(layers), every level of every pyramid stage by stage, layers of 1..4 channels tight and extended, the calls under a
schedule, the ties to the renderer, the scratch reused across level and channel counts, and the plain form of the chain
against the window form.

Shapes (multiband_ref.SHAPES): 9 x 5 -- a coarsest level of 3 x 2, the double fold at n = 2 --, 33 x 17 and 65 x 33 one
column or row past a tile edge at every level, 45 x 27 odd and even sizes in turn, 77 x 41 several tiles in both directions,
150 x 97 five levels and nothing a power of two.  The statement walks the chain once per field in numpy and is shared."""
import functools
import os
import textwrap

import numpy as np
import pytest

import chain_ref
import multiband_ref as MB
import transit_ref
from render_cases import field as _field, frame as _frame, hashes_under_render_mode, layers as _layers, rgb_pair, same_bits as _same
from videomorphing_amd import capi, morph, transition
from videomorphing_amd.multiband import Bands

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GEO = 0.4
EX = 3


def _table(name, L):
    return Bands.linear(L) if name == "linear" else Bands.sharpen(L, 4)


@functools.lru_cache(maxsize=None)
def _maps(w, h, kind, with_path, geo=GEO):
    """(map0, map1) of the uniform chain: walked once per field, shared, never written"""
    v, u = _field(w, h, kind, with_path)
    map0, map1 = MB.warp_ref.sampling_maps(v, u, geo)[:2]
    map0.setflags(write=False)
    map1.setflags(write=False)
    return map0, map1


def _uniform(w, h, kind, with_path, color_fa, geo=GEO):
    map0, map1 = _maps(w, h, kind, with_path, geo)
    return map0, map1, np.full((h, w), f32(color_fa), f32)


# (w, h, L, field, path, table, color_fa): every shape twice, smooth and rough, with and without a path, both tables and the
# three weights several times each; `outside` and `nan` once each at 77 x 41 -- not the full product
WHOLE = [
    (9, 5, 2, "smooth", False, "linear", 0.37), (9, 5, 2, "rough", True, "sharpen", 0.0),
    (33, 17, 2, "smooth", True, "sharpen", 0.37), (33, 17, 2, "rough", False, "linear", 1.0),
    (65, 33, 3, "smooth", False, "sharpen", 1.0), (65, 33, 3, "rough", True, "linear", 0.37),
    (45, 27, 3, "smooth", True, "linear", 0.0), (45, 27, 3, "rough", False, "sharpen", 0.37),
    (77, 41, 4, "smooth", False, "linear", 0.37), (77, 41, 4, "rough", True, "sharpen", 1.0),
    (77, 41, 4, "outside", True, "sharpen", 0.37), (77, 41, 4, "nan", False, "linear", 0.37),
    (150, 97, 5, "smooth", True, "sharpen", 0.37), (150, 97, 5, "rough", False, "linear", 0.0),
]


@pytest.mark.parametrize("w,h,L,kind,with_path,table,color_fa", WHOLE)
def test_whole_calls_equal_the_statement(gpu_ctx, w, h, L, kind, with_path, table, color_fa):
    """the RGB8 call byte for byte -- a NaN pixel is byte 0 on both sides -- and a layer call bit for bit, a NaN for a NaN"""
    v, u = _field(w, h, kind, with_path)
    fr = _frame(gpu_ctx, w, h, EX, v, u)
    bands = _table(table, L)
    maps = _uniform(w, h, kind, with_path, color_fa)
    got = fr.render_multiband(bands, color_fa, GEO)
    want = MB.render_bytes(fr.download_ext(1), fr.download_ext(2), EX, maps, bands.sharp)
    assert got.shape == (h, w, 3) and np.array_equal(got, want), int((got != want).sum())
    ch = (w + L) % 4 + 1
    l0, l1 = _layers(w, h, ch, 10 + ch), _layers(w, h, ch, 20 + ch)
    fr.upload_layers(l0, l1)
    got = fr.render_multiband_layers(bands, color_fa, GEO)
    want = MB.render_layers(l0, l1, maps, bands.sharp)
    assert got.shape == l0.shape and _same(got, want), (ch, int((got != want).sum()))
    fr.close()


@pytest.mark.parametrize("w,h,L,layer_ch", [(45, 27, 3, 0), (150, 97, 5, 0), (45, 27, 3, 4), (150, 97, 5, 2)])
def test_every_level_of_every_stage(gpu_ctx, w, h, L, layer_ch):
    """after one call every Gaussian level of both plates and of the weight, and R at every level, bit for bit: a failure
    names the kernel (warp pass: level 0 of G0, G1, MASK; reduce: the levels above; collapse: OUT) and the level.  Under the
    two_halves colour schedule, so that the weight plane is no constant"""
    v, u = _field(w, h, "smooth", True)
    sched = transit_ref.two_halves(w, h)
    fr = _frame(gpu_ctx, w, h, EX, v, u, (None, sched))
    bands = Bands.sharpen(L, 4)
    maps = MB.scheduled_inputs(v, u, None, sched, 0.5, capi.EASE_LINEAR)
    if layer_ch:
        l0, l1 = _layers(w, h, layer_ch, 3), _layers(w, h, layer_ch, 4)
        fr.upload_layers(l0, l1)
        out = fr.render_multiband_transition_layers(bands, 0.5)
        c0, c1 = MB.layer_plates(l0, l1, maps[0], maps[1])
    else:
        out = fr.render_multiband_transition(bands, 0.5)
        c0, c1 = MB.canvas_plates(fr.download_ext(1), fr.download_ext(2), EX, maps[0], maps[1])
    want = MB.stages(c0, c1, maps[2], bands.sharp)
    names = {capi.MB_G0: "G0", capi.MB_G1: "G1", capi.MB_MASK: "MASK", capi.MB_OUT: "OUT"}
    for what in (capi.MB_G0, capi.MB_G1, capi.MB_MASK, capi.MB_OUT):
        for l in range(L + 1):
            if what == capi.MB_OUT and l == 0 and not layer_ch:
                continue
            got = fr.multiband_level(what, l)
            ref = want[what, l]
            assert got.shape == ref.shape and _same(got, ref), (names[what], l, int((got != ref).sum()))
    if layer_ch:
        assert _same(out, want[MB.OUT, 0])
    else:
        assert np.array_equal(out, chain_ref.bytes_of(want[MB.OUT, 0], True))
        with pytest.raises(capi.VmError) as e:
            fr.multiband_level(capi.MB_OUT, 0)
        assert e.value.code == capi.VM_E_INVALID
    fr.close()


@pytest.mark.parametrize("c", [1, 2, 3, 4])
def test_layers_of_one_to_four_channels(gpu_ctx, c):
    w, h, L = 65, 33, 3
    v, u = _field(w, h, "rough", True)
    fr = _frame(gpu_ctx, w, h, EX, v, u)
    l0, l1 = _layers(w, h, c, 30 + c), _layers(w, h, c, 40 + c)
    fr.upload_layers(l0, l1)
    for table, color_fa in (("linear", 0.37), ("sharpen", 0.5)):
        bands = _table(table, L)
        got = fr.render_multiband_layers(bands, color_fa, GEO)
        want = MB.render_layers(l0, l1, _uniform(w, h, "rough", True, color_fa), bands.sharp)
        assert got.shape == l0.shape and _same(got, want), (table, int((got != want).sum()))
    fr.close()


def test_layer_calls_sample_the_extension(gpu_ctx):
    """after vm_frame_extend_layers the plates are tapped on the extended grid, the image at (ex, ex)"""
    w, h, L, c = 65, 33, 3, 2
    v, _ = _field(w, h, "outside", False)
    fr = morph.Frame(gpu_ctx, w, h, EX)
    fr.upload(None, None, v, None)
    rng = np.random.RandomState(7)
    l0, l1 = rng.rand(h, w, c).astype(f32), rng.rand(h, w, c).astype(f32)
    fr.upload_layers(l0, l1)
    bands = Bands.sharpen(L, 4)
    maps = _uniform(w, h, "outside", False, 0.37)
    tight = fr.render_multiband_layers(bands, 0.37, GEO)
    assert _same(tight, MB.render_layers(l0, l1, maps, bands.sharp))
    fr.extend_layers(1e-6)
    got = fr.render_multiband_layers(bands, 0.37, GEO)
    assert _same(got, MB.render_layers(fr.download_layers_ext(1), fr.download_layers_ext(2), maps, bands.sharp, EX))
    assert not _same(got, tight), "the field's samples leave the image: the extension shows"
    fr.close()


def test_the_plate_as_a_float_layer_gives_the_rgb8_calls_bytes(gpu_ctx):
    """ex = 0: the canvases are the images, and the three-channel layer call on the images as floats forms the RGB8 call's
    R; its bytes after the RGB8 tail are the RGB8 call's"""
    w, h, L = 77, 41, 4
    v, u = _field(w, h, "smooth", True)
    fr = _frame(gpu_ctx, w, h, 0, v, u)
    rgb0, rgb1 = rgb_pair(w, h)
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))
    for bands in (Bands.linear(L), Bands.sharpen(L, 4)):
        assert np.array_equal(chain_ref.bytes_of(fr.render_multiband_layers(bands, 0.37, GEO), True), fr.render_multiband(bands, 0.37, GEO))
    fr.close()


def _scheduled_case(gpu_ctx, w, h, L, sched, t, ease, bands):
    v, u = _field(w, h, "smooth", True)
    fr = _frame(gpu_ctx, w, h, EX, v, u, sched)
    maps = MB.scheduled_inputs(v, u, sched[0], sched[1], t, ease)
    got = fr.render_multiband_transition(bands, t, ease)
    want = MB.render_bytes(fr.download_ext(1), fr.download_ext(2), EX, maps, bands.sharp)
    assert np.array_equal(got, want), int((got != want).sum())
    l0, l1 = _layers(w, h, 3, 5), _layers(w, h, 3, 6)
    fr.upload_layers(l0, l1)
    got = fr.render_multiband_transition_layers(bands, t, ease)
    assert _same(got, MB.render_layers(l0, l1, maps, bands.sharp))
    fr.close()


def test_two_halves_as_the_colour_schedule(gpu_ctx):
    w, h, L = 77, 41, 4
    _scheduled_case(gpu_ctx, w, h, L, (None, transit_ref.two_halves(w, h)), 0.5, capi.EASE_LINEAR, Bands.sharpen(L, 4))


@pytest.mark.parametrize("t", [0.25, 0.5])
@pytest.mark.parametrize("ease", [capi.EASE_LINEAR, capi.EASE_SMOOTH])
def test_a_wipe_as_both_schedules(gpu_ctx, t, ease):
    w, h, L = 45, 27, 3
    wipe = np.ascontiguousarray(transition.wipe(w, h), dtype=f32)
    _scheduled_case(gpu_ctx, w, h, L, (wipe, wipe), t, ease, Bands.linear(L) if ease == capi.EASE_LINEAR else Bands.sharpen(L, 4))


def test_the_uniform_schedule_gives_the_uniform_calls_bits(gpu_ctx):
    w, h, L = 65, 33, 3
    v, u = _field(w, h, "smooth", True)
    fr = _frame(gpu_ctx, w, h, EX, v, u, (transition.uniform(w, h), None))
    l0, l1 = _layers(w, h, 2, 8), _layers(w, h, 2, 9)
    fr.upload_layers(l0, l1)
    bands = Bands.sharpen(L, 4)
    for t in (0.0, 0.37, 1.0):
        assert np.array_equal(fr.render_multiband_transition(bands, t, capi.EASE_LINEAR), fr.render_multiband(bands, t, t))
        assert _same(fr.render_multiband_transition_layers(bands, t, capi.EASE_LINEAR), fr.render_multiband_layers(bands, t, t))
    fr.close()


def test_on_a_zero_field_the_endpoints_are_the_renderers_plates(gpu_ctx):
    """a zero field: the plates are the images (integer-valued), and a weight of 0 (or 1) reconstructs c0 (or c1): the
    bytes of vm_render_halfway with color_from = 0 (or 2)"""
    w, h, L = 77, 41, 4
    zero = np.zeros((h, w, 2), f32)
    fr = _frame(gpu_ctx, w, h, EX, zero, None)
    for bands in (Bands.linear(L), Bands.sharpen(L, 4)):
        assert np.array_equal(fr.render_multiband(bands, 0.0, GEO), fr.render_halfway(0.0, GEO, 0))
        assert np.array_equal(fr.render_multiband(bands, 1.0, GEO), fr.render_halfway(1.0, GEO, 2))
    fr.close()


def test_the_scratch_is_reused_across_levels_and_channels(gpu_ctx):
    """on one frame L = 4, then L = 2, then L = 4 with another channel count: each the bits of a fresh frame; after the
    L = 2 call the diagnostic refuses level 3, before any call it answers VM_E_STATE"""
    w, h = 77, 41
    v, u = _field(w, h, "rough", True)
    lay = {c: (_layers(w, h, c, 50 + c), _layers(w, h, c, 60 + c)) for c in (2, 4)}

    def fresh(L, c):
        fr = _frame(gpu_ctx, w, h, EX, v, u)
        fr.upload_layers(*lay[c])
        out = fr.render_multiband(Bands.sharpen(L, 4), 0.37, GEO), fr.render_multiband_layers(Bands.sharpen(L, 4), 0.37, GEO)
        fr.close()
        return out

    fr = _frame(gpu_ctx, w, h, EX, v, u)
    with pytest.raises(capi.VmError) as e:
        fr.multiband_level(capi.MB_G0, 0)
    assert e.value.code == capi.VM_E_STATE
    for L, c in ((4, 2), (2, 2), (4, 4)):
        fr.upload_layers(*lay[c])
        got = fr.render_multiband(Bands.sharpen(L, 4), 0.37, GEO), fr.render_multiband_layers(Bands.sharpen(L, 4), 0.37, GEO)
        want = fresh(L, c)
        assert np.array_equal(got[0], want[0]) and _same(got[1], want[1]), (L, c)
        if L == 2:
            assert fr.multiband_level(capi.MB_OUT, 2).shape == (11, 20, 2)
            with pytest.raises(capi.VmError) as e:
                fr.multiband_level(capi.MB_G0, 3)
            assert e.value.code == capi.VM_E_INVALID
    fr.close()


_PROG = textwrap.dedent("""
    import hashlib, sys
    import numpy as np
    sys.path.insert(0, %r)
    sys.path.insert(0, %r)
    import warp_ref, transit_ref
    from videomorphing_amd import capi, morph, synth
    from videomorphing_amd.multiband import Bands
    ctx = morph.Context(0, capi.MATH_FAST)
    for w, h, L, kind in ((150, 97, 5, "smooth"), (77, 41, 4, "nan"), (9, 5, 2, "rough")):
        rgb0, rgb1 = synth.make_rgb_pair(w, h)
        rng = np.random.RandomState(41)
        v, u = warp_ref.field(kind, w, h, rng), warp_ref.path(w, h, rng)
        fr = morph.Frame(ctx, w, h, 3)
        for path in (None, u):
            hh = hashlib.sha256()
            fr.upload(morph.make_extended(rgb0, 3), morph.make_extended(rgb1, 3), v, path)
            fr.upload_schedule(None, transit_ref.two_halves(w, h))
            fr.upload_layers(rgb0.astype(np.float32) / np.float32(3), rgb1.astype(np.float32))
            bands = Bands.sharpen(L, 4)
            hh.update(fr.render_multiband(bands, 0.37, 0.4).tobytes())
            hh.update(fr.render_multiband_transition(bands, 0.5).tobytes())
            for lay in (fr.render_multiband_layers(bands, 0.37, 0.4), fr.render_multiband_transition_layers(bands, 0.5)):
                nan = np.isnan(lay)                 # a NaN for a NaN: its sign and payload are not specified
                hh.update(nan.tobytes())
                hh.update(np.where(nan, np.float32(0), lay).tobytes())
            print("HASH", w, h, kind, path is not None, hh.hexdigest())
        fr.close()
""") % (ROOT, os.path.join(ROOT, "tests"))


def test_both_forms_of_the_chain_agree(gpu_ctx):
    """the plain gather kernels (VM_RENDER=plain) give the window kernels' bits: a fresh child process under each hashes
    three calls' worth of outputs -- uniform and scheduled, bytes and layers -- with and without a path"""
    plain, window = hashes_under_render_mode(_PROG, "plain"), hashes_under_render_mode(_PROG, None)
    assert len(window) == 6
    assert plain == window, [a for a, b in zip(plain, window) if a != b]
