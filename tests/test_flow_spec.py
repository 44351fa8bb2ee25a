"""The dense optical flow's spec (tests/flow_ref.py) checked on the CPU, and the flow
C-ABI's host-side contract (defaults, struct layout, argument checks before any device work)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import flow_ref as R
from videomorphing_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# interior endpoint-error bounds (16-px border excluded) of the analytic-flow checks, shared with
# tests/test_gpu_flow.py; measured with flow_ref at 320 x 192, frames 0 -> 1 and 1 -> 0:
#   shift (0.5, 0.25):  median 0.022 / 0.019 px, 95th percentile 0.048 / 0.041 px
#   shift (6.0, -3.5):  median 0.025 / 0.024 px, 95th percentile 0.058 / 0.053 px
EPE_MEDIAN, EPE_P95 = 0.05, 0.15


def test_separable_polynomial_expansion_equals_a_direct_fit():
    rng = np.random.default_rng(7)
    img = rng.random((20, 24)) * 255
    for n, sigma in ((5, 1.1), (7, 1.5)):
        a, b = R.poly_exp(img, n, sigma), R.poly_exp_direct(img, n, sigma)
        assert np.abs(a - b).max() < 1e-9, (n, np.abs(a - b).max())


def test_scale_table():
    t = R.scales(1920, 1080)
    assert len(t) == 6 and (t[-1][1], t[-1][2]) == (60, 34)
    assert [(w, h) for _, w, h in R.scales(100, 70)] == [(100, 70), (50, 35)]
    assert len(R.scales(32, 32)) == 1


def test_grey_constants():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255]]], np.uint8)
    assert R.grey(rgb).tolist() == [[76.0, 150.0, 29.0, 255.0]]
    v = np.arange(256, dtype=np.uint8)[None]
    assert np.array_equal(R.grey(np.stack([v, v, v], -1))[0], np.arange(256.0))


def test_blur_sizes():
    assert len(R.blur_taps(0.5)) == 3 and len(R.blur_taps(0.5 ** 5)) == 79
    assert abs(R.blur_taps(0.25).sum() - 1) < 1e-12


def test_identical_frames_give_zero_flow():
    a, _ = synth.make_video_pair(96, 64, 0)
    assert np.abs(R.flow(a, a)).max() == 0


@pytest.mark.parametrize("shift", [(0.5, 0.25), (6.0, -3.5)])
def test_translating_video_meets_the_bounds(shift):
    """measured: see EPE_MEDIAN / EPE_P95 above"""
    w, h = 320, 192
    a, _ = synth.make_video_pair(w, h, 0, shift)
    b, _ = synth.make_video_pair(w, h, 1, shift)
    for d, truth in ((R.flow(a, b), shift), (R.flow(b, a), (-shift[0], -shift[1]))):
        e = R.endpoint_error(d, truth)
        assert np.median(e) <= EPE_MEDIAN and np.percentile(e, 95) <= EPE_P95, (np.median(e), np.percentile(e, 95))


def test_params_default(vmlib):
    p = capi.FlowParams()
    assert vmlib.vm_flow_params_default(C.byref(p)) == capi.VM_OK
    assert (p.num_levels, p.pyr_scale, p.fast_pyramids, p.win_size, p.num_iters, p.poly_n, p.flags) == (5, 0.5, 0, 13, 10, 5, 0)
    assert abs(p.poly_sigma - 1.1) < 1e-6
    assert vmlib.vm_flow_params_default(None) == capi.VM_E_INVALID


def test_flow_params_layout(tmp_path):
    prog = tmp_path / "fp.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vmorph.h"\nint main(void){printf("%zu %zu %zu\\n",'
                    'sizeof(vm_flow_params),offsetof(vm_flow_params,poly_sigma),offsetof(vm_flow_params,flags));return 0;}\n')
    exe = tmp_path / "fp"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(capi.FlowParams), capi.FlowParams.poly_sigma.offset, capi.FlowParams.flags.offset] == [32, 24, 28]


def _bad_params():
    out = []
    for k, v in (("fast_pyramids", 1), ("flags", 256), ("flags", 4), ("win_size", 12), ("win_size", 33), ("win_size", 1),
                 ("poly_n", 6), ("poly_n", 3), ("poly_sigma", 0.0), ("pyr_scale", 1.0), ("pyr_scale", 0.0), ("num_iters", 0),
                 ("num_levels", -1)):
        p = capi.FlowParams()
        capi.load().vm_flow_params_default(C.byref(p))
        setattr(p, k, v)
        out.append(p)
    return out


def test_bad_arguments_are_rejected_before_any_device_work(vmlib):
    """NULL handles and out-of-range parameters come back as VM_E_INVALID with a message, with no
    context at all (no device is touched: this runs on a machine without a GPU)"""
    a = np.zeros((40, 40), np.float32)
    o = np.zeros((40, 40, 2), np.float32)
    pa = (C.c_void_p * 1)(a.ctypes.data)
    po = (C.c_void_p * 1)(o.ctypes.data)
    assert vmlib.vm_optical_flow_luma(None, 40, 40, 1, pa, pa, 0, None, po) == capi.VM_E_INVALID
    assert vmlib.vm_optical_flow_rgb(None, 40, 40, 1, pa, pa, 0, None, po) == capi.VM_E_INVALID
    assert vmlib.vm_video_build_flows_rgb(None, pa, pa, 0, None) == capi.VM_E_INVALID
    assert vmlib.vm_sync_compute_flows(None, None) == capi.VM_E_INVALID
    assert vmlib.vm_last_error()
    # a non-null but unusable context pointer is never dereferenced before the parameters are checked
    bogus = C.c_void_p(16)
    for p in _bad_params():
        assert vmlib.vm_optical_flow_luma(bogus, 40, 40, 1, pa, pa, 0, C.byref(p), po) == capi.VM_E_INVALID
        assert b"flow" in vmlib.vm_last_error()
    for w, h in ((31, 40), (40, 31), (0, 0)):
        assert vmlib.vm_optical_flow_luma(bogus, w, h, 1, pa, pa, 0, None, po) == capi.VM_E_INVALID


# ---- the float32 spec, the flip-excused share, the scale table and the arguments of the stage tests
# (tests/test_gpu_flow_stages.py, cases in tests/flow_cases.py) -----------------------------------------

def test_float32_spec_holds_no_float64_array():
    """a dtype=float32 run keeps every array and intermediate float32: at every return of a flow_ref
    function no float array among its locals or its result is wider.  The constants are computed in
    float64 (gauss_taps, blur_taps, poly_inverse) and rounded once (in poly_consts and blur)."""
    import sys
    import flow_cases as FC
    constants = {"gauss_taps", "blur_taps", "poly_inverse", "poly_consts", "scales", "check_params", "flip_eps", "f32"}
    wide, seen = [], set()

    def look(frame, event, arg):
        code = frame.f_code
        if event != "return" or code.co_filename != R.__file__ or code.co_name in constants:
            return
        seen.add(code.co_name)
        for name, v in list(frame.f_locals.items()) + [("<result>", arg)]:
            for x in (v if isinstance(v, (list, tuple)) else [v]):
                if isinstance(x, (np.ndarray, np.generic)) and x.dtype.kind == "f" and x.dtype != np.float32:
                    wide.append((code.co_name, name, x.dtype))

    a, b = FC.frames("edge", 5, 70, 48)
    p = FC.spec_params(dict(num_levels=1, num_iters=2, pyr_scale=0.7, poly_n=7, poly_sigma=1.5))
    sys.setprofile(look)
    try:
        d32 = R.flow(a, b, p, np.float32)
    finally:
        sys.setprofile(None)
    assert {"flow", "iterate", "poly_exp", "blur", "resize", "_box", "_axis", "scale_images"} <= seen
    assert not wide, wide
    d64 = R.flow(a, b, p)
    assert d32.dtype == np.float32 and d64.dtype == np.float64
    dist = np.abs(d32 - d64).max()
    assert 0 < dist < 1e-3 * np.abs(d64).max(), dist  # float32 arithmetic, and nothing coarser


def test_float64_is_the_default_and_rgb_goes_through_grey():
    import flow_cases as FC
    a, b = FC.rgb_frames("rgb", 3, 48, 40)
    p = R.params(num_levels=0, num_iters=2)
    assert np.array_equal(R.flow(a, b, p), R.flow(R.grey(a), R.grey(b), p, np.float64))
    d, mask = R.flow(a, b, p, excuse=True)
    assert np.array_equal(d, R.flow(a, b, p)) and mask.shape == d.shape[:2] and mask.dtype == bool


def test_flip_distance_and_excused_mask():
    """iterate(dist=True): the distance of x + d to the thresholds 0, w - 1, h - 1; none where d is 0"""
    h, w = 40, 48
    rng = np.random.default_rng(4)
    Pa, Pb = R.poly_exp(rng.random((h, w)) * 255), R.poly_exp(rng.random((h, w)) * 255)
    d = np.zeros((h, w, 2))
    out, dist = R.iterate(Pa, Pb, d, 5, dist=True)
    assert np.isinf(dist).all() and np.array_equal(out, R.iterate(Pa, Pb, d, 5))
    d[10, 44, 0] = 3.0 - 1e-5     # x + d = w - 1 - 1e-5
    d[0, 20, 1] = 2e-4            # y + d = 2e-4
    d[30, 10] = (1.5, -2.25)
    dist = R.iterate(Pa, Pb, d, 5, dist=True)[1]
    assert abs(dist[10, 44] - 1e-5) < 1e-12 and abs(dist[0, 20] - 2e-4) < 1e-12 and dist[30, 10] == 11.25
    assert np.isinf(dist).sum() == h * w - 3
    assert R.flip_eps(w, h) == 64 * 2.0 ** -18  # 64 ulps of 47
    m = np.zeros((h, w), bool)
    m[10, 44] = True
    g = R._dilate(m, 2)
    assert g.sum() == 25 and g[8:13, 42:47].all()
    assert R._dilate(np.pad(np.ones((1, 1), bool), ((0, 5), (0, 5))), 3).sum() == 16   # clipped at the frame
    up = R._resize_mask(m, 2 * w, 2 * h)
    assert up[20:22, 88:90].all() and 4 <= up.sum() <= 16 and not up[:18].any()


def _case_ids():
    import flow_cases as FC
    return dict(argvalues=FC.CASES + FC.BIG, ids=FC.IDS + [c[0] for c in FC.BIG])


@pytest.mark.parametrize("case", **_case_ids())
def test_excused_share_of_the_stage_cases(case):
    """the float64 spec alone keeps every seeded case within the cap: at most 1 % of the pixels within
    reach of a flip candidate, none for the num_iters = 1 cases; and no case is degenerate"""
    import flow_cases as FC
    _, kind, seed, w, h, kw = case
    a, b = FC.frames(kind, seed, w, h)
    d, mask = R.flow(a, b, FC.spec_params(kw), excuse=True)
    assert mask.mean() <= FC.excused_cap(case), (case[0], mask.mean())
    if kind in ("const", "same"):
        assert not d.any()
    else:
        assert np.abs(d).max() > 0.5, np.abs(d).max()


def _exact_scales(w, h, num_levels, pyr_scale):
    """DESIGN 3.6's rule in exact rational arithmetic on the float32 value the library holds"""
    from fractions import Fraction
    ps, out = Fraction(float(np.float32(pyr_scale))), []
    for k in range(num_levels + 1):
        s = ps ** k
        if w * s < 32 or h * s < 32:
            break
        out.append(tuple(int(round(n * s)) for n in (w, h)))  # Fraction rounds half to even, as rint does
    return out


@pytest.mark.parametrize("w,h,pyr_scale", [(100, 70, 0.5), (65, 70, 0.7), (115, 120, 0.3), (40, 44, 0.8), (50, 50, 0.8),
                                           (200, 200, 0.16), (83, 70, 0.8), (1600, 1600, 0.02), (1664, 1664, 0.02),
                                           (257, 64, 0.7), (1920, 1080, 0.5), (64, 63, 0.5), (55, 64, 0.7)])
def test_scale_table_of_the_float32_pyr_scale(w, h, pyr_scale):
    """flow_ref.scales, given the float32-rounded pyr_scale (the host's pow((double)pyr_scale, k)),
    states the table of the exact rule; the double of the same decimal can state another one"""
    got = [(wk, hk) for _, wk, hk in R.scales(w, h, 9, R.f32(pyr_scale))]
    assert got == _exact_scales(w, h, 9, pyr_scale)


def test_scale_table_cases_where_the_double_differs():
    sizes = lambda w, h, s: [(wk, hk) for _, wk, hk in R.scales(w, h, 1, s)]
    assert sizes(65, 70, R.f32(0.7)) == [(65, 70), (45, 49)] and sizes(65, 70, 0.7) == [(65, 70), (46, 49)]
    assert sizes(115, 120, R.f32(0.3))[1] == (35, 36) and sizes(115, 120, 0.3)[1] == (34, 36)
    assert len(sizes(200, 200, R.f32(0.16))) == 1 and len(sizes(200, 200, 0.16)) == 2
    assert len(sizes(1600, 1600, R.f32(0.02))) == 1 and sizes(1664, 1664, R.f32(0.02))[1] == (33, 33)
    assert sizes(40, 44, R.f32(0.8))[1] == (32, 35)


def _flow_args(n=40):
    a = np.zeros((n, n), np.float32)
    o = np.zeros((n, n, 2), np.float32)
    return a, o, (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(o.ctypes.data)


def test_pitch_below_the_row_is_rejected(vmlib):
    """with no device: a pitch below the row is VM_E_INVALID by its own message; 0 and any pitch from
    the row up pass the check and the call goes on to reject the unusable context"""
    a, o, pa, po = _flow_args()
    bogus = C.c_void_p(16)
    for fn, row in ((vmlib.vm_optical_flow_luma, 40), (vmlib.vm_optical_flow_rgb, 120)):
        for pitch in (row - 1, 1, -row):
            assert fn(bogus, 40, 40, 1, pa, pa, pitch, None, po) == capi.VM_E_INVALID
            assert b"pitch" in vmlib.vm_last_error()
        for pitch in (0, row, row + 7):
            assert fn(bogus, 40, 40, 1, pa, pa, pitch, None, po) == capi.VM_E_INVALID
            assert b"pitch" not in vmlib.vm_last_error() and b"context" in vmlib.vm_last_error()


def _fp(**kw):
    p = capi.FlowParams()
    capi.load().vm_flow_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_blur_radius_limit(vmlib):
    """a scale whose blur radius is above 96 px is rejected before any device work, by the library and by
    flow_ref.check_params alike; radius 96 passes parameter resolution"""
    a, o, pa, po = _flow_args()
    bogus = C.c_void_p(16)
    cases = [(8192, 8192, dict(num_levels=8), False),
             (8192, 8192, dict(num_levels=5), True),            # radius 39 at the deepest scale
             (2600, 2600, dict(num_levels=1, pyr_scale=0.0128), True),    # radius 96
             (2600, 2600, dict(num_levels=1, pyr_scale=0.01275), False),  # radius 97
             (2600, 2600, dict(num_levels=0, pyr_scale=0.01275), True),   # the scale is never built
             (2400, 2600, dict(num_levels=1, pyr_scale=0.01275), True)]   # 2400 * 0.01275 < 32: no such scale
    assert len(R.blur_taps(R.f32(0.0128))) // 2 == 96 and len(R.blur_taps(R.f32(0.01275))) // 2 == 97
    assert R.MAX_BLUR_R == 96
    for w, h, kw, ok in cases:
        rc = vmlib.vm_optical_flow_luma(bogus, w, h, 1, pa, pa, 0, C.byref(_fp(**kw)), po)
        msg = vmlib.vm_last_error()
        assert rc == capi.VM_E_INVALID
        assert (b"blur radius" not in msg and b"context" in msg) if ok else b"blur radius" in msg, (w, h, kw, msg)
        p = R.params(**kw)
        p["pyr_scale"] = R.f32(p["pyr_scale"])
        if ok:
            R.check_params(p, w, h)
        else:
            with pytest.raises(ValueError, match="blur radius"):
                R.check_params(p, w, h)


def test_chunk_formula_at_1080p():
    """the pairs per chunk the GPU chunk-boundary test relies on (vm_flow.h: 4 GiB, 20 B per pixel of
    every scale per frame, 24 B per full-resolution pixel per flow)"""
    frame = sum(wk * hk * 20 for _, wk, hk in R.scales(1920, 1080))
    assert [(wk, hk) for _, wk, hk in R.scales(1920, 1080)][-2:] == [(120, 68), (60, 34)]
    assert int((4 << 30) / (2.0 * frame + 1920 * 1080 * 24)) == 26
