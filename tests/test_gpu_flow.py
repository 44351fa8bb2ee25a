"""Dense optical flow on the GPU (vm_flow.hip; MdiEditor::OpticalFlow, UI/MdiEditor.cpp:1584-1689)
against its CPU statement (tests/flow_ref.py) and against the analytic flows of the translating
synthetic videos; batch invariance; the video and sync entry points against the upload paths they
replace; an end-to-end video solve on computed flows."""
import ctypes as C

import numpy as np
import pytest

import flow_ref as R
from test_flow_spec import EPE_MEDIAN, EPE_P95, _bad_params
from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu

# GPU (float32) against flow_ref (float64): measured RMS <= 6.1e-7 px, max <= 4.8e-6 px over the three
# cases of test_gpu_matches_the_cpu_spec; the bounds are about ten times that
REF_RMS, REF_MAX = 5e-6, 5e-5


def _frames(w, h, t0, t1, shift=(0.5, 0.25)):
    return synth.make_video_pair(w, h, t0, shift)[0], synth.make_video_pair(w, h, t1, shift)[0]


def _textured(w, h, t, shift, base=40.0):
    """frame t of a video translating by `shift` px per frame, with the noise texture of a 320-px
    synth.make_video_pair frame at any size (make_video_pair scales its texture with the frame: at
    1080p it is so smooth that A'A stays far below the 1e-3 regulariser of the solve and the method
    itself, flow_ref included, returns almost no motion)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    n = synth.value_noise(x - shift[0] * t, y - shift[1] * t, base)
    top = 2.0 - 0.5 ** (synth.OCTAVES - 1)
    lo, hi = 0.25 * top, 0.75 * top
    return np.clip(16.0 + (n - lo) / (hi - lo) * 224.0, 16.0, 240.0).astype(np.float32)


def _rgb(luma):
    v = np.clip(np.rint(luma), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(np.stack([v, v, v], -1))


@pytest.mark.parametrize("w,h,kw", [(192, 120, {}), (127, 99, {}), (192, 120, dict(win_size=7, poly_n=7, poly_sigma=1.5, num_levels=2))])
def test_gpu_matches_the_cpu_spec(gpu_ctx, w, h, kw):
    a, b = _frames(w, h, 0, 1, (1.5, -0.75))
    p = R.params(**kw)
    want = R.flow(a, b, p)
    got = morph.optical_flow(gpu_ctx, a, b, morph.FlowParams(**kw))[0]
    d = np.abs(got - want)
    rms = np.sqrt((d ** 2).mean())
    print("%dx%d %s: rms %.3g max %.3g" % (w, h, kw, rms, d.max()))
    assert rms <= REF_RMS and d.max() <= REF_MAX, (rms, d.max())
    # RGB8 input: a grey (v, v, v) frame is the luma frame v
    ar, br = _rgb(a), _rgb(b)
    got_rgb = morph.optical_flow(gpu_ctx, ar, br, morph.FlowParams(**kw))[0]
    got_l = morph.optical_flow(gpu_ctx, ar[..., 0].astype(np.float32), br[..., 0].astype(np.float32), morph.FlowParams(**kw))[0]
    assert np.array_equal(got_rgb.view(np.uint32), got_l.view(np.uint32))


@pytest.mark.parametrize("w,h,shift,tex", [(640, 360, (0.5, 0.25), False), (640, 360, (6.0, -3.5), True),
                                           (1920, 1080, (6.0, -3.5), True)])
def test_accuracy_against_the_analytic_flow(gpu_ctx, w, h, shift, tex):
    """the bounds of the CPU check; flow_ref on the same frames measured median 0.033 / 0.025 / 0.025 px,
    95th percentile 0.080 / 0.058 / 0.058 px"""
    a, b = (_textured(w, h, 0, shift), _textured(w, h, 1, shift)) if tex else _frames(w, h, 0, 1, shift)
    e = R.endpoint_error(morph.optical_flow(gpu_ctx, a, b)[0], shift)
    print("%dx%d %s: median %.4f p95 %.4f" % (w, h, shift, np.median(e), np.percentile(e, 95)))
    assert np.median(e) <= EPE_MEDIAN and np.percentile(e, 95) <= EPE_P95


def test_batch_invariance(gpu_ctx):
    w, h = 200, 136
    frames = [synth.make_video_pair(w, h, t, (1.0, 0.5))[0] for t in range(13)]
    a, b = np.stack(frames[:-1]), np.stack(frames[1:])
    one = morph.optical_flow(gpu_ctx, a[5], b[5])[0]
    batch = morph.optical_flow(gpu_ctx, a, b)
    again = morph.optical_flow(gpu_ctx, a, b)
    assert np.array_equal(one.view(np.uint32), batch[5].view(np.uint32))
    assert np.array_equal(batch.view(np.uint32), again.view(np.uint32))
    assert np.abs(batch).max() > 0.3


def test_backward_is_minus_forward(gpu_ctx):
    w, h, d = 160, 96, 4
    v0 = np.stack([synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25))[0] for t in range(d)])
    v1 = np.stack([synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25))[1] for t in range(d)])
    f0, f1, b0, b1 = morph.video_optical_flows(gpu_ctx, v0, v1)
    assert not f0[-1].any() and not b0[0].any() and not f1[-1].any() and not b1[0].any()
    for t in range(d - 1):
        for f, b in ((f0, b0), (f1, b1)):
            dd = np.abs(b[t + 1] + f[t])[16:-16, 16:-16]
            assert np.median(dd) < 0.05 and np.percentile(dd, 95) < 0.2, (t, np.median(dd), np.percentile(dd, 95))
    assert np.median(np.abs(f0[0] - np.float32([0.5, 0.25]))[16:-16, 16:-16]) < 0.05


def test_video_build_flows_rgb_equals_host_flows(gpu_ctx):
    w, h, d = 96, 64, 5
    s0, s1 = (0.5, 0.25), (1.5, -0.25)
    fr = [synth.make_video_pair(w, h, t, s0, s1) for t in range(d)]
    rgb0, rgb1 = np.stack([_rgb(f[0]) for f in fr]), np.stack([_rgb(f[1]) for f in fr])
    # the host path: flows out, vm_video_build_flows in
    a = np.concatenate([rgb0[:-1], rgb1[:-1], rgb0[1:], rgb1[1:]])
    b = np.concatenate([rgb0[1:], rgb1[1:], rgb0[:-1], rgb1[:-1]])
    fl = morph.optical_flow(gpu_ctx, a, b)
    m = d - 1
    fam = [np.zeros((d, h, w, 2), np.float32) for _ in range(4)]
    fam[0][:-1], fam[1][:-1], fam[2][1:], fam[3][1:] = fl[:m], fl[m:2 * m], fl[2 * m:3 * m], fl[3 * m:]
    levels, factor_t = synth.video_levels(w, h, d, 16)
    host, dev = morph.VideoPyramid(gpu_ctx), morph.VideoPyramid(gpu_ctx)
    host.build_levels(levels, factor_t, d)
    dev.build_levels(levels, factor_t, d)
    host.build_flows(*fam)
    dev.build_flows_rgb(rgb0, rgb1)
    for l in range(len(levels) - 1):
        for t in range(levels[l][2]):
            for name in ("f0", "f1", "b0", "b1"):
                x, y = host.pages[l][t].field(name), dev.pages[l][t].field(name)
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (l, t, name)
    assert np.abs(dev.pages[0][1].field("f1")).max() > 1.0


def test_sync_compute_flows_equals_upload(gpu_ctx):
    w, h, d = 96, 64, 4
    fr = [synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25)) for t in range(d)]
    v0 = np.stack([_rgb(f[0]) for f in fr])
    v1 = np.stack([_rgb(f[1]) for f in fr])
    zero = np.zeros((d, h, w, 2), np.float32)
    f0, f1, _, _ = morph.video_optical_flows(gpu_ctx, v0, v1)
    up, comp = morph.SyncPyramid(gpu_ctx), morph.SyncPyramid(gpu_ctx)
    up.build(v0, v1, f0, f1, 16)
    comp.build(v0, v1, zero, zero, 16)
    comp.compute_flows()
    for fa, frame in ((0.5, 1), (0.25, 2), (0.75, 0)):
        assert np.array_equal(up.render_resample(fa, frame), comp.render_resample(fa, frame)), (fa, frame)


def test_video_solve_on_computed_flows(gpu_ctx):
    """end to end: a 5-frame 320 x 192 pair solved (FAST, w_temp 10) on flows computed on the device
    (VideoPyramid.build_rgb) against the same solve on the analytic flows: measured mean distance of the
    halfway fields <= 0.0124 px per page, temp_mask coverage of the outer pages 1.0 (analytic: 0.997)"""
    w, h, d = 320, 192, 5
    s0, s1 = (0.5, 0.25), (1.5, -0.25)
    fr = [synth.make_video_pair(w, h, t, s0, s1) for t in range(d)]
    rgb0, rgb1 = np.stack([_rgb(f[0]) for f in fr]), np.stack([_rgb(f[1]) for f in fr])
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    res, cover = {}, {}
    try:
        for mode in ("computed", "analytic"):
            prm = morph.Parameters()
            prm.max_iter, prm.max_iter_drop_factor, prm.start_res, prm.w_temp = 12, 1.0, 32, 10.0
            vid = morph.VideoPyramid(gpu_ctx)
            if mode == "computed":
                vid.build_rgb(rgb0, rgb1, 32)
            else:
                levels, factor_t = synth.video_levels(w, h, d, 32)
                vid.build_levels(levels, factor_t, d)
                for t in range(d):
                    vid.build_rgb_frame(t, rgb0[t], rgb1[t])
                vid.build_flows(*synth.constant_flows(w, h, d, s0, s1))
            vm = morph.VideoMorph(prm, vid)
            vm.calculate_halfway_parametrization()
            res[mode] = [vid.pages[0][t].v for t in range(len(vid.pages[0]))]
            cover[mode] = [(vid.pages[0][t].field("temp_mask") > 0).mean() for t in (0, len(vid.pages[0]) - 1)]
            del vid
    finally:
        gpu_ctx.set_math_mode(capi.MATH_EXACT)
    dist = [np.sqrt(((a - b) ** 2).sum(-1)).mean() for a, b in zip(res["computed"], res["analytic"])]
    print("mean distance per page", dist, "coverage", cover)
    assert max(dist) <= 0.05, dist  # measured: at most 0.0124 px
    assert min(cover["computed"]) >= min(cover["analytic"]) - 0.01, cover
    assert max(np.abs(v).max() for v in res["computed"]) > 0.2


def test_bad_parameters_on_a_device(gpu_ctx):
    a = np.zeros((1, 64, 64), np.float32)
    for p in _bad_params():
        with pytest.raises(capi.VmError) as e:
            morph.optical_flow(gpu_ctx, a, a, p)
        assert e.value.code == capi.VM_E_INVALID
    small = np.zeros((1, 31, 64), np.float32)
    with pytest.raises(capi.VmError) as e:
        morph.optical_flow(gpu_ctx, small, small)
    assert e.value.code == capi.VM_E_INVALID
    sp = morph.SyncPyramid(gpu_ctx)
    sp.build_levels(morph.sync_level_table(64, 48, 3, 16))
    with pytest.raises(capi.VmError) as e:  # no frame uploaded yet
        sp.compute_flows()
    assert e.value.code == capi.VM_E_STATE
