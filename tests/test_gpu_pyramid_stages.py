"""The device pyramid builder (vm_pyramid.hip, the flow half of vm_temporal.hip, Builder in
vm_pyramid_api.cpp) by stage, at full size and at its edges.

(a) Reductions (k_down, k_tri_solve: no powf) through vm_dbg_pyramid_scale against the oracle's
    vmo_scale_planes, bit for bit: output lines of 1 to 1920 samples on either axis around the 32-sample
    register chunks of the solve, line counts around the 64-line workgroup, 3840x2160 -> 1920x1080, the
    ratios 2:1 (even and odd), 3:1, 200 -> 67, 5 -> 4 and n + 1 -> n, both sides and the tie of the
    axis-order rule.
(b) Same size and enlargement (k_curve, k_tri_solve, k_up, k_curve: powf) against the float64 statement
    tests/pyramid_ref.py.  Bound, per case: D = max |oracle - float64|; the device must stay within 4 D of
    float64.  Device and oracle are two float32 roundings of one real-valued function, so each sits about D
    from float64; 4 leaves a factor of two.  Nothing on the path is discontinuous (the support weights go
    to zero at their limits, clamp and curves are continuous): no pixel is excused.
(c) Whole chains through vm_pyramid_build_rgb / vm_video_build_rgb with the bound of (b) per level:
    1920x1080x6 and 3840x2160x7 against the oracle live, the smallest pyramids vm_pyramid_create admits,
    a row pitch of 3 w + 7, a frame that hits both branches of both curves and the clamp.
(d) Flows through vm_video_build_flows with the bound of (b) in px: amplitudes 40 and 80 (saturation at
    50 px x ratio), 161x91 frames, a temporal pyramid whose concatenation leaves the frame on every side
    and meets whole-number displacements, one 1080p level, and a level LARGER than the one before it (the
    x ratio rule's other branch; the builder's buffers are sized by the largest level of the chain).

MEASURED on an MI355X (D: smallest .. largest over the cases of a group; ratio = max |device - float64| / D,
largest and median over the cases; the bound is 4):
  (a) reductions, 80 cases                        bit for bit in all 80, 3840x2160 -> 1920x1080 among them
  (b) same size, 39 cases          planes         D 3.6e-07 .. 7.3e-05    ratio 1.18 (7x63), median 1.00
  (b) enlargement / mixed, 9       planes         D 2.0e-07 .. 8.0e-05    ratio 1.05, median 1.00
  (c) 1920x1080x6                  luma 0..255    D 6.3e-05 .. 6.1e-04    ratio 1.24 (level 6), median 1.00
  (c) 3840x2160x7                  luma           D 6.7e-05 .. 6.3e-04    ratio 1.07, median 1.00
  (c) 129x33x4, 80x5x1             luma           D 6.3e-05 .. 5.3e-04    ratio 1.11, median 1.00
  (c) black next to saturated      luma           D 6.5e-05 .. 3.4e-03    ratio 1.01, median 1.00
  (d) amplitude 40 / 80            px             D 1.2e-05 .. 4.0e-05    ratio 1.10 / 1.05
  (d) 161x91                       px             D 1.7e-05 .. 2.4e-05    ratio 1.50, median 1.31
  (d) factor_t = 2 (concatenated)  px             D 2.4e-05 .. 2.5e-04    ratio 2.41 (level 1, b0), median 1.11
  (d) one 1080p level              px             D 4.9e-07 .. 4.0e-05    ratio 1.00
  (d) a level that grows           px             D 2.0e-05 .. 7.7e-05    ratio 1.47, median 1.07
  (c) a level that grows           luma           D 4.3e-05 .. 1.2e-03    ratio 1.12, median 1.00
A ratio of 1.00 means the device's worst sample is the oracle's: the device's powf agrees with libm's on almost
every sample, and where no powf is involved (a) the two agree in every bit.  The row-pitch test holds bit for bit.

One-line mutations of the kernels and of Builder, one library build each, against this module: a wrong factor index in
the chunk loop, a dropped prefetch hand-over in the backward pass, a mirror off by one, no normalisation by the weight
sum, no clamp in k_flow_store, `<=` in the axis-order rule and a tight row pitch in k_load each fail between 1 and 139
tests; "always x ratio" in k_flow_store fails the growing-level test only.  `0.5f + o` for `0.5 + o` in k_down passes
everything and must: o + 0.5 is exact in float32, and the float32 difference of two float32 numbers is the rounding
of their exact difference, which is what the double expression rounds to as well.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyramid_cases as PC
import pyramid_ref as R
from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu

CHUNK_EDGES = [1, 2, 3, 31, 32, 33, 34, 63, 64, 65, 66, 96, 97, 960, 1920]
LINE_COUNTS = [63, 64, 65, 129]


def _reductions():
    """(w, h, wout, hout), both axes shrink"""
    cases = []
    for n in CHUNK_EDGES:
        cases.append((2 * n, 14, n, 7))                  # the tie of the axis order: rows first
        cases.append((14, 2 * n, 7, n))
        if n > 1:
            cases.append((2 * n - 1, 13, n, 7))          # odd -> n
            cases.append((13, 2 * n - 1, 7, n))
    for l in LINE_COUNTS:
        cases.append((80, l, 40, (l + 1) // 2))          # the row solve runs on l lines
        cases.append((l, 80, (l + 1) // 2, 40))          # the column solve runs on l lines
    cases += [(3840, 2160, 1920, 1080),
              (192, 120, 64, 40), (200, 120, 67, 40), (120, 200, 40, 67), (5, 5, 4, 4), (50, 40, 40, 32),
              (34, 33, 33, 32), (98, 66, 97, 65), (2, 2, 1, 1), (7, 5, 4, 3), (4, 3, 2, 2), (257, 3, 129, 2),
              (80, 40, 40, 20), (1921, 1081, 961, 541)]
    return cases


def _same_or_larger():
    cases = []
    for n in CHUNK_EDGES:
        cases += [(n, 7, n, 7), (7, n, 7, n)]
    for l in LINE_COUNTS:
        cases += [(80, l, 80, l), (l, 80, l, 80)]
    cases += [(1920, 1080, 1920, 1080), (3840, 2160, 3840, 2160),
              (64, 40, 100, 70), (40, 64, 70, 100), (33, 32, 34, 33), (96, 64, 97, 65), (1, 1, 2, 2), (2, 1, 3, 2),
              (2, 1, 1, 1), (65, 30, 33, 30), (30, 65, 30, 33)]          # one axis shrinks, the other goes through powf
    return cases


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _dev_scale(ctx, p, wo, ho):
    p = np.ascontiguousarray(p, dtype=np.float32)
    _, h, w = p.shape
    out = np.full((3, ho, wo), np.nan, dtype=np.float32)
    capi.check(capi.load().vm_dbg_pyramid_scale(ctx._h, p.ctypes.data, w, h, wo, ho, out.ctypes.data))
    return out


def _within(label, dev, orc, f64):
    """the bound of (b): D = max |oracle - float64|, device within 4 D of float64.  Prints the figures first."""
    D = float(np.abs(orc.astype(np.float64) - f64).max())
    e = float(np.abs(dev.astype(np.float64) - f64).max())
    print("%-44s D %.3e  device %.3e  ratio %s" % (label, D, e, ("%.2f" % (e / D)) if D > 0 else "-"))
    assert np.isfinite(dev).all()
    assert e <= 4 * D, (label, e, D)
    return D, e


@pytest.mark.parametrize("w,h,wo,ho", _reductions())
def test_reductions_equal_the_oracle_bit_for_bit(gpu_ctx, oracle, w, h, wo, ho):
    p = PC.noise_planes(w, h, 7 * w + h)
    got, want = _dev_scale(gpu_ctx, p, wo, ho), oracle.scale_planes(p, wo, ho)
    same = np.array_equal(_bits(got), _bits(want))
    if not same:
        d = np.abs(got - want)
        print("%dx%d -> %dx%d differs: max %.3e at %s, %d of %d samples" % (w, h, wo, ho, d.max(), np.unravel_index(d.argmax(), d.shape), (d > 0).sum(), d.size))
    assert same
    assert w * h < 100 or (p.min() < 0 and p.max() > 1 and np.ptp(want) > 1)


def test_the_axis_order_shows_in_the_bits(gpu_ctx, oracle):
    """the rule `hout * w < wout * h` picks the first axis; the two orders differ in the last bits only, so the three
    cases above (either side and the tie) pin it only because they are compared bit for bit: the other order of the
    oracle's own operations does not give the device's bits"""
    for w, h, wo, ho in ((200, 120, 67, 40), (120, 200, 40, 67), (80, 40, 40, 20)):
        p = PC.noise_planes(w, h, 7 * w + h)
        got = _dev_scale(gpu_ctx, p, wo, ho)
        first = 0 if R.columns_first(w, h, wo, ho) else 1           # the axis the rule does NOT start with
        other = R.scale_axis(R.scale_axis(p, (wo, ho)[first], first, np.float32), (wo, ho)[1 - first], 1 - first, np.float32)
        assert not np.array_equal(_bits(got), _bits(other)) and np.abs(got - other).max() < 1e-5


def test_scale_rejects_bad_sizes(gpu_ctx):
    L = capi.load()
    p = np.zeros((3, 4, 4), np.float32)
    assert L.vm_dbg_pyramid_scale(gpu_ctx._h, p.ctypes.data, 4, 4, 0, 4, p.ctypes.data) == capi.VM_E_INVALID
    assert L.vm_dbg_pyramid_scale(gpu_ctx._h, p.ctypes.data, 4, 0, 4, 4, p.ctypes.data) == capi.VM_E_INVALID
    assert L.vm_dbg_pyramid_scale(gpu_ctx._h, None, 4, 4, 4, 4, p.ctypes.data) == capi.VM_E_INVALID
    assert L.vm_dbg_pyramid_scale(None, p.ctypes.data, 4, 4, 4, 4, p.ctypes.data) == capi.VM_E_INVALID


@pytest.mark.parametrize("w,h,wo,ho", _same_or_larger())
def test_same_size_and_enlargement_within_float32_of_the_statement(gpu_ctx, oracle, w, h, wo, ho):
    p = PC.noise_planes(w, h, 7 * w + h)
    got, orc, f64 = _dev_scale(gpu_ctx, p, wo, ho), oracle.scale_planes(p, wo, ho), R.scale(p, wo, ho)
    _within("scale %dx%d -> %dx%d" % (w, h, wo, ho), got, orc, f64)
    if (wo, ho) == (w, h) and w * h > 1:
        assert np.abs(got - p).max() < 1e-4 < np.ptp(got)        # prefilter + reconstruction at phase 0: the identity


# ---- (c) whole chains -----------------------------------------------------------------------------------------

def _sizes(w, h, n):
    out = [(w, h)]
    for _ in range(n - 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def _padded(rgb, pitch, fill=0xAB):
    h, w = rgb.shape[:2]
    buf = np.full((h, pitch), fill, dtype=np.uint8)
    buf[:, :3 * w] = rgb.reshape(h, 3 * w)
    return buf


def _build_rgb(ctx, sizes, rgb0, rgb1, pitch=0):
    """vm_pyramid_build_rgb on explicit level sizes (the last one holds no images): [(img0, img1)] per image level"""
    pyr = morph.Pyramid(ctx)
    pyr.build_levels(sizes)
    a, b = (np.ascontiguousarray(x, dtype=np.uint8) for x in (rgb0, rgb1))
    if pitch:
        a, b = _padded(a, pitch), _padded(b, pitch, 0x5C)
    capi.check(pyr._L.vm_pyramid_build_rgb(pyr._h, a.ctypes.data, b.ctypes.data, pitch))
    return [(pyr[el].field("img0"), pyr[el].field("img1")) for el in range(1, len(sizes))]


@functools.lru_cache(maxsize=None)
def _frames(w, h):
    return PC.harsh_rgb(w, h, w + h), synth.make_rgb_pair(w, h)[1]


@pytest.mark.parametrize("w,h,nl", [(1920, 1080, 6), (3840, 2160, 7)])
def test_full_size_luma_pyramid_against_the_oracle_live(gpu_ctx, oracle, w, h, nl):
    rgb = _frames(w, h)
    lum = _build_rgb(gpu_ctx, _sizes(w, h, nl + 1), *rgb)
    for k in range(2):
        orc, f64 = oracle.luma_pyramid(rgb[k], nl), R.luma_pyramid(rgb[k], nl)
        for el in range(nl):
            assert lum[el][k].shape == orc[el].shape
            _within("luma %dx%d frame %d level %d" % (w, h, k, el + 1), lum[el][k], orc[el], f64[el])
    assert np.ptp(lum[0][0]) > 250                        # black and saturated pixels are in the frame


@pytest.mark.parametrize("sizes,more", [
    ([(129, 33), (65, 17), (33, 9), (17, 5), (9, 5)], [(129, 33), (65, 17), (33, 9), (17, 5), (9, 3)]),
    ([(80, 5), (40, 5)], [(80, 5), (40, 3)]),
])
def test_smallest_pyramids(gpu_ctx, oracle, sizes, more):
    """vm_pyramid_create admits no level under 5 x 5: the smallest image levels the public entry reaches, and
    VM_E_INVALID for the next ceil-halved level (shorter lines are reached through vm_dbg_pyramid_scale above)"""
    w, h = sizes[0]
    nl = len(sizes) - 1
    rgb = PC.harsh_rgb(w, h, 3), PC.harsh_rgb(w, h, 4)
    lum = _build_rgb(gpu_ctx, sizes, *rgb)
    for k in range(2):
        orc, f64 = oracle.luma_pyramid(rgb[k], nl), R.luma_pyramid(rgb[k], nl)
        for el in range(nl):
            assert lum[el][k].shape == orc[el].shape == (sizes[el][1], sizes[el][0])
            _within("luma %dx%d frame %d level %d" % (w, h, k, el + 1), lum[el][k], orc[el], f64[el])
    n = len(more)
    hnd = C.c_void_p()
    rc = capi.load().vm_pyramid_create(gpu_ctx._h, n, (C.c_int * n)(*[s[0] for s in more]), (C.c_int * n)(*[s[1] for s in more]), C.byref(hnd))
    assert rc == capi.VM_E_INVALID and not hnd.value


def test_row_pitch_gives_the_bits_of_the_tight_call(gpu_ctx):
    w, h = 333, 61
    rgb = PC.harsh_rgb(w, h, 9), synth.make_rgb_pair(w, h)[1]
    sizes = _sizes(w, h, 4)
    tight, pitched = _build_rgb(gpu_ctx, sizes, *rgb), _build_rgb(gpu_ctx, sizes, *rgb, pitch=3 * w + 7)
    for a, b in zip(tight, pitched):
        for k in range(2):
            assert np.array_equal(_bits(a[k]), _bits(b[k])) and np.ptp(a[k]) > 100
    # the video entry
    levels = [(s[0], s[1], 2) for s in sizes]
    out = []
    for pitch in (0, 3 * w + 7):
        dev = morph.VideoPyramid(gpu_ctx)
        dev.build_levels(levels, [1] * 4, 2)
        for t in range(2):
            a, b = rgb[t], rgb[1 - t]
            if pitch:
                a, b = _padded(a, pitch), _padded(b, pitch, 0x5C)
            capi.check(dev._L.vm_video_build_rgb(dev._h, t, a.ctypes.data, b.ctypes.data, pitch))
        out.append([dev.pages[l][t].field(f) for l in range(3) for t in range(2) for f in ("img0", "img1")])
    for a, b in zip(*out):
        assert np.array_equal(_bits(a), _bits(b)) and np.ptp(a) > 100
    for l in range(3):                                   # ... and it is the frame-pair entry's pyramid
        assert np.array_equal(_bits(out[0][4 * l]), _bits(tight[l][0]))
    assert capi.load().vm_video_build_rgb(dev._h, 0, rgb[0].ctypes.data, rgb[1].ctypes.data, 3 * w - 1) == capi.VM_E_INVALID


def test_both_branches_of_both_curves_and_the_clamp(gpu_ctx, oracle):
    """a frame with values on either side of the curves' linear segments and black blocks next to saturated ones: the
    B-spline inverse overshoots below 0 and above 1 there, so store_gray clamps on both sides"""
    w, h, nl = 257, 131, 4
    rgb = PC.harsh_rgb(w, h, 21), PC.harsh_rgb(w, h, 22)
    assert (rgb[0] <= 10).any() and (rgb[0] == 11).any() and (rgb[0] == 0).any() and (rgb[0] == 255).any()
    img = R.scale(R.load(rgb[0]), (w + 1) // 2, (h + 1) // 2)
    assert img.min() < -0.01 and img.max() > 1.01 and (np.abs(img) < 0.0031308).any()
    lum = _build_rgb(gpu_ctx, _sizes(w, h, nl + 1), *rgb)
    for k in range(2):
        orc, f64 = oracle.luma_pyramid(rgb[k], nl), R.luma_pyramid(rgb[k], nl)
        for el in range(nl):
            _within("harsh frame %d level %d" % (k, el + 1), lum[el][k], orc[el], f64[el])
            assert lum[el][k].min() >= 0 and lum[el][k].max() <= 255.001
    assert lum[1][0].min() == 0 and lum[1][0].max() > 254.99


# ---- (d) flows ------------------------------------------------------------------------------------------------

def _flow_check(ctx, O, label, levels, ft, fam):
    """vm_video_build_flows against oracle.flow_pyramids with the bound of (b), in px; returns the device's pages"""
    dev = morph.VideoPyramid(ctx)
    dev.build_levels(levels, ft, levels[0][2])
    dev.build_flows(*fam)
    orc = O.flow_pyramids(fam[0], fam[1], fam[2], fam[3], levels, ft)
    f64 = R.flow_pyramids(fam[0], fam[1], fam[2], fam[3], levels, ft)
    got = []
    for l in range(len(levels) - 1):
        got.append({})
        for k in ("f0", "f1", "b0", "b1"):
            got[l][k] = [dev.pages[l][t].field(k) for t in range(levels[l][2])]
            a, b, c = (np.stack(x[l][k]) for x in (got, orc, f64))
            _within("%s level %d %s" % (label, l, k), a, b, c)
    return got, orc


def _family(w, h, d, amp, seed):
    return [[PC.smooth_flow(w, h, amp, seed + 10 * k + t) for t in range(d)] for k in range(4)]


@pytest.mark.parametrize("amp", [40.0, 80.0])
def test_flows_at_and_beyond_the_range(gpu_ctx, oracle, amp):
    levels, ft = [(160, 90, 2), (80, 45, 2), (40, 23, 2)], [1, 1, 1]
    got, _ = _flow_check(gpu_ctx, oracle, "flows amp %g" % amp, levels, ft, _family(160, 90, 2, amp, 300))
    for l, ratio in ((0, 1.0), (1, 0.5)):
        a = np.abs(got[l]["f0"][0])
        assert a.max() <= 50 * ratio + 1e-4
        if amp > 50:                                      # the plateau at 50 px x ratio is reached on the device too
            assert (a > 50 * ratio - 1e-3).mean() > 0.05


def test_flows_of_odd_frames(gpu_ctx, oracle):
    levels, ft = [(161, 91, 2), (81, 46, 2), (41, 23, 2)], [1, 1, 1]
    _flow_check(gpu_ctx, oracle, "flows 161x91", levels, ft, _family(161, 91, 2, 6.0, 400))


def test_concatenated_flows_leave_the_frame_and_meet_whole_numbers(gpu_ctx, oracle):
    """factor_t = 2 at the first reduced level: its flows are scaled from full-resolution flows, so a region beyond
    -50 px comes out at exactly -25.0 px (the lower clamp is exact) and the concatenation samples at whole-number
    positions there (floor == ceil); large flows near the border leave the frame on every side"""
    levels, ft = [(96, 64, 5), (48, 32, 3), (24, 16, 3)], [1, 2, 1]
    fam = _family(96, 64, 5, 30.0, 500)
    for k in range(4):
        for t in range(5):
            fam[k][t][20:40, 30:60] = (-60.0, -75.0)
            fam[k][t][44:60, 4:24] = (70.0, 55.0)
    pre = oracle.flow_scale(fam[0][0], 48, 32)             # what the concatenation starts from
    y, x = np.mgrid[0:32, 0:48]
    px, py = x + pre[..., 0], y + pre[..., 1]
    assert (px < 0).any() and (px > 47).any() and (py < 0).any() and (py > 31).any()
    assert ((pre[..., 0] == -25.0) & (pre[..., 1] == -25.0)).sum() > 50
    got, orc = _flow_check(gpu_ctx, oracle, "flows factor_t 2", levels, ft, fam)
    assert np.abs(orc[1]["f0"][0] - pre).max() > 5         # level 1 really is concatenated


def test_flows_of_one_1080p_level(gpu_ctx, oracle):
    """two frames, the same-size level of a 1080p video (lines of 1920 and 1080 samples through the solve on the flow
    path).  One field of every family, both frames among them, is compared; the device builds all eight."""
    w, h = 1920, 1080
    levels, ft = [(w, h, 2), (960, 540, 2)], [1, 1]
    fam = _family(w, h, 2, 45.0, 600)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, ft, 2)
    dev.build_flows(*fam)
    for k, name, t in ((0, "f0", 0), (1, "f1", 1), (2, "b0", 1), (3, "b1", 0)):
        _within("flows 1080p %s[%d]" % (name, t), dev.pages[0][t].field(name), oracle.flow_scale(fam[k][t], w, h), R.flow_scale(fam[k][t], w, h))


def test_flows_through_a_level_that_grows(gpu_ctx, oracle):
    """vm_video_create admits a level larger than the one before it.  The flow rule then differs: a flow is multiplied
    by the size ratios only when one of them is below 1 -- by both of them then, also by the one above 1 (level 2 here),
    and by neither when both sides grow (level 1).  The builder's buffers are sized by the largest level."""
    levels, ft = [(64, 40, 2), (100, 70, 2), (50, 80, 2), (25, 40, 2)], [1, 1, 1, 1]
    got, orc = _flow_check(gpu_ctx, oracle, "flows growing level", levels, ft, _family(64, 40, 2, 12.0, 700))
    a, b = np.abs(orc[0]["f0"][0]).mean(), np.abs(orc[1]["f0"][0]).mean()
    assert 0.8 * a < b < 1.25 * a                          # enlarged, not rescaled
    y1, y2 = np.abs(orc[1]["f0"][0][..., 1]).mean(), np.abs(orc[2]["f0"][0][..., 1]).mean()
    assert 0.97 * 80 / 70 < y2 / y1 < 1.03 * 80 / 70       # x shrinks, so y is multiplied by its ratio above 1 too


def test_luma_pyramid_through_a_level_that_grows(gpu_ctx, oracle):
    """the image half with a level larger than the frame (k_up at a real ratio through the public entry).  The oracle's
    luma chain only halves, so the float32 side of the yardstick is oracle.scale_planes between the statement's own
    load and store_gray"""
    sizes = [(64, 40), (100, 70), (50, 35), (25, 18)]
    rgb = PC.harsh_rgb(64, 40, 31), synth.make_rgb_pair(64, 40)[1]
    lum = _build_rgb(gpu_ctx, sizes, *rgb)
    for k in range(2):
        a32, a64 = R.load(rgb[k], np.float32), R.load(rgb[k])
        for el, (w, h) in enumerate(sizes[:-1]):
            a32, a64 = oracle.scale_planes(a32, w, h), R.scale(a64, w, h)
            _within("growing luma frame %d level %d" % (k, el + 1), lum[el][k], R.store_gray(a32, np.float32), R.store_gray(a64))
