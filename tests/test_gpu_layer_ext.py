"""The Poisson extension of float layers (videomorphing_amd/csrc/vm_layer_ext.hip, vm_frame_extend_layers;
PoissonExt.cpp:49-362) on the GPU, against tests/layer_ext_ref.py: the stages bit for bit, the solution against the
float64 statement, the tie to the pinned RGB path, the edge cases, the ordered mode, the render calls on extended layers
bit for bit, and the refusals.

The solution's bound.  Measured on an MI355X at tol = 1e-6 (profiles/layer_extension.md lists every case): the largest
absolute deviation from the float64 statement over all cases, layers in [0, 1] (the HDR case, drawn in [0, 1000], divided
by 1000), is MEASURED_MAX.  The bound is four times that -- the margin for the run-to-run order of the atomics and for
another batch shape -- and has to stay below 1e-3 of the value range, or the extension is not right yet."""
import numpy as np
import pytest

import layer_ext_ref as R
import shutter_ref
import viewport_ref
from layer_ext_cases import CHANNELS, CONSTANTS, KINDS, SHAPES, field, layers, reference
from render_cases import rgb_pair as _rgb, same_bits as _same
from videomorphing_amd import capi, morph
from videomorphing_amd.viewport import Viewport

pytestmark = pytest.mark.gpu

f32 = np.float32
TOL = 1e-6
MEASURED_MAX = 2.601e-6    # 138x84x8, v = (0, -4), 3 channels (profiles/layer_extension.md)
BOUND = 4 * MEASURED_MAX
FIELDS = KINDS + sorted(CONSTANTS)
shapes = pytest.mark.parametrize("w,h,ex", SHAPES)
fields = pytest.mark.parametrize("kind", FIELDS)
channels = pytest.mark.parametrize("c", CHANNELS)


def _frame(ctx, w, h, ex, kind, lay):
    fr = morph.Frame(ctx, w, h, ex)
    fr.upload(None, None, field(w, h, kind), None)
    if lay is not None:
        fr.upload_layers(*lay)
    return fr


def test_the_bound_meets_the_issues_condition():
    assert 0 < BOUND < 1e-3


@shapes
@fields
@channels
def test_stages_equal_the_statement(gpu_ctx, w, h, ex, kind, c):
    """1: the filled canvas, valid, the type map and the right-hand side (the statement's expression in float32) of both
    sides, bit for bit; the call leaves the frame as it was"""
    l0, l1 = layers(w, h, c, 7)
    fr = _frame(gpu_ctx, w, h, ex, kind, (l0, l1))
    before = fr.render_layers(0.3, 0.5, 1)
    for side, own, other in ((1, l0, l1), (2, l1, l0)):
        filled, valid, typ = R.prepare(own, other, field(w, h, kind), ex, side)
        got = fr.layers_prepare(side)
        assert _same(got[0], filled), (side, "filled")
        assert np.array_equal(got[1], valid), (side, "valid")
        assert np.array_equal(got[2], typ), (side, "type")
        assert _same(got[3], R.rhs(filled, valid, typ, f32)), (side, "rhs")
    assert _same(fr.render_layers(0.3, 0.5, 1), before)
    fr.close()


def _deviation(fr, w, h, ex, kind, c, seed, scale=1.0):
    """the largest |device - float64 statement| over both sides, in units of the value range; asserts that the interior
    keeps the uploaded bits"""
    l = layers(w, h, c, seed, scale)
    worst = 0.0
    for side in (1, 2):
        ref, typ = reference(w, h, ex, kind, c, seed, scale)[side - 1]
        got = fr.download_layers_ext(side)
        inner = typ == 0
        assert _same(got[inner], l[side - 1][inner[ex:ex + h, ex:ex + w]]), "interior cells keep the uploaded bits"
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()) / scale)
    return worst


@shapes
@fields
@channels
def test_solution_meets_the_float64_statement(gpu_ctx, w, h, ex, kind, c):
    """2: at tol = 1e-6, within four times the largest recorded deviation"""
    fr = _frame(gpu_ctx, w, h, ex, kind, layers(w, h, c, 7))
    res, _ = fr.extend_layers(TOL)
    assert len(res) == (c + 2) // 3 and all(rel <= TOL for g in res for _, rel in g)
    dev = _deviation(fr, w, h, ex, kind, c, 7)
    print("DEV %dx%dx%d %s C=%d %.3e" % (w, h, ex, kind, c, dev))
    assert dev <= BOUND
    fr.close()


def test_solution_of_an_hdr_layer(gpu_ctx):
    """2: values drawn in [0, 1000], the deviation divided by 1000"""
    w, h, ex = SHAPES[0]
    fr = _frame(gpu_ctx, w, h, ex, "smooth", layers(w, h, 3, 11, 1000.0))
    fr.extend_layers(TOL)
    dev = _deviation(fr, w, h, ex, "smooth", 3, 11, 1000.0)
    print("DEV %dx%dx%d smooth C=3 hdr %.3e" % (w, h, ex, dev))
    assert dev <= BOUND
    fr.close()


@shapes
@pytest.mark.parametrize("kind", ["zero"] + sorted(CONSTANTS))
def test_integer_layers_floor_to_the_rgb_canvases(gpu_ctx, w, h, ex, kind):
    """3: the layer is the frame's RGB as floats; floor(clip(extended layer, 0, 255)) against poisson_extend_both's canvas of
    the same frame: no byte further than one level (the hole guess is 0 here and 128 there, the RGB fill rounds to bytes)"""
    rgb0, rgb1 = _rgb(w, h)
    fr = morph.Frame(gpu_ctx, w, h, ex)
    fr.upload_rgb(rgb0, rgb1)
    fr.upload(None, None, field(w, h, kind), None)
    fr.upload_layers(rgb0.astype(f32), rgb1.astype(f32))
    fr.poisson_extend_both(TOL)
    fr.extend_layers(TOL)
    differ = total = 0
    for side in (1, 2):
        rgb = fr.download_ext(side)[..., :3].astype(np.int64)
        lay = np.floor(np.clip(fr.download_layers_ext(side), 0, 255)).astype(np.int64)
        assert np.abs(lay - rgb).max() <= 1, side
        differ += int((lay != rgb).sum())
        total += rgb.size
    print("RGBTIE %dx%dx%d %s %.4f%% of the bytes differ by one level" % (w, h, ex, kind, 100.0 * differ / total))
    fr.close()


@shapes
def test_zero_and_constant_layers(gpu_ctx, w, h, ex):
    """4: an all-zero layer extends to exact zeros without a solve; so does the zero fourth channel of a 4-channel layer; a
    constant layer stays within the bound of check 2"""
    fr = _frame(gpu_ctx, w, h, ex, "smooth", None)
    z = np.zeros((h, w, 1), f32)
    fr.upload_layers(z, z)
    res, _ = fr.extend_layers(TOL)
    assert res == [((0, 0.0), (0, 0.0))]
    for side in (1, 2):
        assert not fr.download_layers_ext(side).view(np.uint32).any()
    l0, l1 = (np.array(a) for a in layers(w, h, 4, 7))
    l0[..., 3] = l1[..., 3] = 0
    fr.upload_layers(l0, l1)
    res, _ = fr.extend_layers(TOL)
    assert res[1] == ((0, 0.0), (0, 0.0)) and res[0][0][0] > 0
    for side in (1, 2):
        assert not fr.download_layers_ext(side)[..., 3].view(np.uint32).any()
    const = np.full((h, w, 3), 0.625, f32)
    fr.upload_layers(const, const)
    fr.extend_layers(TOL)
    for side in (1, 2):
        assert np.abs(fr.download_layers_ext(side).astype(np.float64) - 0.625).max() <= BOUND
    fr.close()


@pytest.mark.parametrize("w,h,ex", SHAPES[:3])
def test_ordered_mode_gives_the_same_bits(vmlib, w, h, ex):
    """5: under VM_REDUCE_ORDERED two runs and a fresh frame give identical bits"""
    ctx = morph.Context(0)
    try:
        ctx.set_reduction(capi.REDUCE_ORDERED)
        lay = layers(w, h, 4, 7)
        fr = _frame(ctx, w, h, ex, "outside", lay)
        runs = []
        for _ in range(2):
            fr.extend_layers(TOL)
            runs.append([fr.download_layers_ext(s) for s in (1, 2)])
        fresh = _frame(ctx, w, h, ex, "outside", lay)
        fresh.extend_layers(TOL)
        runs.append([fresh.download_layers_ext(s) for s in (1, 2)])
        for other in runs[1:]:
            assert _same(other[0], runs[0][0]) and _same(other[1], runs[0][1])
        fresh.close()
        fr.close()
    finally:
        ctx.close()


@shapes
@pytest.mark.parametrize("kind", ["large", "outside"])
@channels
def test_render_calls_sample_the_extension(gpu_ctx, w, h, ex, kind, c):
    """6: after extension render_layers, render_shutter_layers (1 and 3 samples) and render_viewport_layers (identity, and
    half size with 2 x 2 samples) equal the statement sampling download_layers_ext() at the chain's maps, bit for bit;
    after drop_layer_extension and after a new upload_layers they give the unextended bits again"""
    lay = layers(w, h, c, 7)
    v = field(w, h, kind)
    fr = _frame(gpu_ctx, w, h, ex, kind, lay)
    half = Viewport.fit(w, h, max(w // 2, 1), max(h // 2, 1)).supersampled(2)
    views = (Viewport.identity(w, h), half)

    def calls():
        out = [fr.render_layers(0.3, g, cf) for g in (0.0, 0.5) for cf in (0, 1, 2)]
        out += [fr.render_shutter_layers(0.3, 0.1, 0.9, n, 1) for n in (1, 3)]
        out += [fr.render_viewport_layers(vp, 0.3, 0.5, 1) for vp in views]
        return out

    tight = calls()
    fr.extend_layers(TOL)
    e0, e1 = fr.download_layers_ext(1), fr.download_layers_ext(2)
    want = []
    for g in (0.0, 0.5):
        m0, m1 = fr.sampling_maps(g)[:2]
        want += [R.render_layers(e0, e1, ex, m0, m1, 0.3, cf) for cf in (0, 1, 2)]
    want += [R.layers_on_maps(e0, e1, ex, shutter_ref.sample_maps(v, None, 0.1, 0.9, n), 0.3, 1) for n in (1, 3)]
    want += [R.layers_on_maps(e0, e1, ex, viewport_ref.sample_maps(v, None, 0.5, vp.astuple()), 0.3, 1) for vp in views]
    got = calls()
    for k, (a, b) in enumerate(zip(got, want)):
        assert _same(a, b), k
    assert any(not _same(a, b) for a, b in zip(got, tight)), "the field's samples leave the image: the extension shows"
    fr.drop_layer_extension()
    assert all(_same(a, b) for a, b in zip(calls(), tight))
    fr.extend_layers(TOL)
    fr.upload_layers(*lay)
    assert all(_same(a, b) for a, b in zip(calls(), tight))
    fr.close()


def test_refusals(gpu_ctx):
    """7: the states and arguments of include/vmorph.h; a NaN in a border-ring pixel gives VM_E_NUMERIC and leaves the
    frame rendering its tight layers"""
    w, h, ex = 33, 7, 3
    L = capi.load()
    lay = layers(w, h, 3, 7)
    fr = _frame(gpu_ctx, w, h, ex, "outside", None)
    hnd = fr._h
    ext = lambda tol=TOL, it=100: L.vm_frame_extend_layers(hnd, tol, it, None, None, None)
    out = np.empty((h + 2 * ex, w + 2 * ex, 3), f32)
    assert ext() == capi.VM_E_STATE                                              # no layers
    assert L.vm_dbg_layers_prepare(hnd, 1, None, None, None, None) == capi.VM_E_STATE
    fr.upload_layers(*lay)
    assert L.vm_frame_download_layers_ext(hnd, 1, out.ctypes.data, 0) == capi.VM_E_STATE     # not extended
    assert ext(0.0) == capi.VM_E_INVALID and ext(-1.0) == capi.VM_E_INVALID and ext(TOL, 0) == capi.VM_E_INVALID
    assert ext(float("nan")) == capi.VM_E_INVALID
    assert L.vm_dbg_layers_prepare(hnd, 3, None, None, None, None) == capi.VM_E_INVALID
    assert L.vm_dbg_layers_prepare(hnd, 1, None, None, None, None) == capi.VM_OK  # every output may be NULL
    flat = morph.Frame(gpu_ctx, w, h, 0)
    flat.upload_layers(*lay)
    assert L.vm_frame_extend_layers(flat._h, TOL, 100, None, None, None) == capi.VM_E_STATE  # ex == 0
    flat.close()
    tight = fr.render_layers(0.3, 0.5, 1)
    assert ext(1e-30, 3) == capi.VM_E_NUMERIC                                    # the residual stays above tol
    assert _same(fr.render_layers(0.3, 0.5, 1), tight)
    assert ext() == capi.VM_OK
    assert L.vm_frame_download_layers_ext(hnd, 0, out.ctypes.data, 0) == capi.VM_E_INVALID
    assert L.vm_frame_download_layers_ext(hnd, 1, None, 0) == capi.VM_E_INVALID
    assert L.vm_frame_download_layers_ext(hnd, 1, out.ctypes.data, 3) == capi.VM_E_INVALID   # a pitch below the row
    assert not _same(fr.render_layers(0.3, 0.5, 1), tight)
    bad = np.array(lay[0])
    bad[0, w // 2, 1] = np.nan
    fr.upload_layers(bad, lay[1])
    tight = fr.render_layers(0.3, 0.5, 1)
    assert ext() == capi.VM_E_NUMERIC
    assert _same(fr.render_layers(0.3, 0.5, 1), tight)
    assert L.vm_frame_drop_layer_extension(hnd) == capi.VM_OK                    # a no-op without extension
    fr.close()
