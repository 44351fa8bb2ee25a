"""The optical-flow kernels (vm_flow.hip) stage by stage, at their tile and frame edges, and in colour,
against the CPU statement tests/flow_ref.py on hard inputs (tests/flow_cases.py: white noise, step
edges, sharp blocks, a 12-px motion, a zoom, constant and identical frames).

Short chains through the public entry point isolate the stages: num_levels=0, num_iters=1 is k_poly and
one k_iter at d = 0; num_iters=2 and 3 add the displaced gather and its out-of-frame branch;
num_levels=1, num_iters=1 adds the blur, the resize and the flow upsampling with one coarse iteration
behind them.

Tolerance.  Nothing measured on the kernel enters a bound.  For every case the test computes the spec
twice on the CPU, in float64 and in float32 (flow_ref's dtype switch), and demands
    err_max <= K * dist_max   and   err_rms <= K * dist_rms,    K = 4,
err = |GPU - spec64|, dist = |spec32 - spec64|, over the pixels that are not excused.  Where dist is
exactly 0 (constant or identical frames) the GPU flow must be all-zero bits.  Excused are the pixels a
flip candidate of the float64 run can reach (flow_ref.flow(excuse=True): a sample position within 64
float32 ulps of an `inside` threshold, grown by win/2 per iteration and by the resize footprint per
level); the share is capped at 1 % of a case, 0 for num_iters = 1 (tests/test_flow_spec.py checks the
cap on the CPU).  K covers the kernel's summation order and FMA contraction against numpy's.

Measured ratios err / dist (max-norm, RMS) per case on an MI355X, K = 4 throughout:
    poly-iter0-noise         dist max 1.12e-06 ratio max 0.86 rms 1.00
    poly-iter0-edge          dist max 2.17e-06 ratio max 1.05 rms 0.99
    poly-iter0-blocks        dist max 2.3e-06  ratio max 1.01 rms 1.04
    poly-iter0-large-n7      dist max 9.99e-06 ratio max 0.99 rms 0.90
    gather2-noise            dist max 3.45e-06 ratio max 1.02 rms 1.05
    gather3-noise            dist max 2.19e-06 ratio max 1.09 rms 1.02
    gather2-large            dist max 9.48e-06 ratio max 1.02 rms 1.00
    gather3-large            dist max 1.9e-05  ratio max 1.01 rms 1.00
    gather2-blocks           dist max 2.82e-06 ratio max 2.49 rms 1.11
    gather3-edge             dist max 9.87e-06 ratio max 0.71 rms 0.94
    level1-s0.5-noise        dist max 1.75e-06 ratio max 0.90 rms 0.98
    level1-s0.8-noise        dist max 1.61e-06 ratio max 1.26 rms 1.04
    level1-s0.7-edge         dist max 2.16e-05 ratio max 0.96 rms 1.02
    level1-s0.3-large        dist max 1.79e-05 ratio max 0.87 rms 0.91
    level1-s0.8-at32         dist max 1.95e-06 ratio max 0.82 rms 1.00
    level3-s0.8-noise        dist max 1.75e-06 ratio max 1.16 rms 1.07
    win3-n5-32x32            dist max 8.14e-06 ratio max 1.04 rms 1.04
    win3-n7-33x47            dist max 1.07e-05 ratio max 1.19 rms 0.96
    win13-n7-65x33           dist max 1.35e-06 ratio max 1.03 rms 1.01
    win13-n5-32x32           dist max 4.69e-06 ratio max 1.43 rms 1.06
    win17-n5-257x64          dist max 4.54e-06 ratio max 1.17 rms 1.14
    win17-n7-96x129          dist max 3.61e-05 ratio max 1.30 rms 0.61
    win19-n5-100x70          dist max 1.07e-06 ratio max 1.63 rms 1.13
    win19-n7-40x300          dist max 2.81e-06 ratio max 1.04 rms 0.90
    win31-n5-300x40          dist max 3.52e-06 ratio max 0.79 rms 1.27
    win31-n7-65x33           dist max 1.28e-05 ratio max 1.62 rms 1.60
    win31-n5-32x32           dist max 7.64e-07 ratio max 0.77 rms 0.83
    win17-n5-33x47           dist max 1.69e-05 ratio max 1.00 rms 1.02
    win19-n5-257x64          dist max 2.09e-05 ratio max 1.34 rms 1.06
    levels0-default-iters    dist max 2.7e-06  ratio max 0.85 rms 1.06
    levels9-100x70           dist max 5.44e-06 ratio max 0.53 rms 1.00
    defaults-zoom-192x120    dist max 4.88e-06 ratio max 0.91 rms 1.00
    defaults-zoom-127x99     dist max 4.16e-06 ratio max 0.67 rms 0.96
    blur-r40-1072            dist max 0.000823 ratio max 1.13 rms 1.02
    const, same              dist 0: all-zero bits
    rgb-rgb / red / blue      ratio max 0.98 / 0.95 / 0.96, rms 0.98;  rgb-boundary ratio max 1.14 rms 1.01
No case needed more than K = 4; the largest ratio is 2.49 (gather2-blocks, max-norm).
"""
import ctypes as C

import numpy as np
import pytest

import flow_cases as FC
import flow_ref as R
from videomorphing_amd import capi, morph

pytestmark = pytest.mark.gpu

K = 4.0


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(name, got, d64, d32, mask, cap):
    """the K rule on the pixels outside `mask`"""
    share = mask.mean()
    assert share <= cap, "%s: %.4f of the pixels excused, cap %.2f" % (name, share, cap)
    ok = ~mask
    err = np.abs(got.astype(np.float64) - d64)[ok]
    dist = np.abs(d32.astype(np.float64) - d64)[ok]
    em, er, dm, dr = err.max(), np.sqrt((err ** 2).mean()), dist.max(), np.sqrt((dist ** 2).mean())
    if dm == 0:
        print("FLOWCASE %s: dist 0, excused %.4f, GPU max |d| %g" % (name, share, np.abs(got).max()))
        assert not _bits(got).any(), "%s: the spec is exactly 0 in both precisions, the GPU flow is not" % name
        return
    print("FLOWCASE %s: err max %.3g rms %.3g  dist max %.3g rms %.3g  ratio max %.2f rms %.2f  excused %.4f  |d| max %.3g"
          % (name, em, er, dm, dr, em / dm, er / dr, share, np.abs(d64).max()))
    assert em <= K * dm and er <= K * dr, "%s: err max %.3g rms %.3g against dist max %.3g rms %.3g" % (name, em, er, dm, dr)


@pytest.mark.parametrize("case", FC.CASES, ids=FC.IDS)
def test_stage_case_against_the_spec(gpu_ctx, case):
    a, b, d64, mask, d32 = FC.reference(case)
    got = morph.optical_flow(gpu_ctx, a, b, morph.FlowParams(**case[5]))[0]
    assert got.shape == d64.shape
    _check(case[0], got, d64, d32, mask, FC.excused_cap(case))


def test_large_radius_blur(gpu_ctx):
    """radius 40 (81 taps, 36.3 KB of dynamic LDS in k_blur_cols) in front of a 32 x 32 level"""
    case = FC.BIG[0]
    assert len(R.blur_taps(R.f32(case[5]["pyr_scale"]))) // 2 == 40
    a, b, d64, mask, d32 = FC.reference(case)
    got = morph.optical_flow(gpu_ctx, a, b, morph.FlowParams(**case[5]))[0]
    _check(case[0], got, d64, d32, mask, FC.excused_cap(case))


@pytest.mark.parametrize("w,h,pyr_scale,depth", [
    (100, 70, 0.5, 1),     # 50 x 35, then 25 < 32
    # the depth is pinned here, not the level sizes: 45 against 46 px and 35 against 34 px are told apart by the
    # K-rule cases level1-s0.7-edge and level1-s0.3-large of flow_cases (a coarse level one px off moves the flow
    # by far more than 4 x dist); keep those two cases
    (65, 70, 0.7, 1),      # 65 * f32(0.7) = 45.4999992: 45 wide (46 with the double 0.7)
    (115, 120, 0.3, 1),    # 115 * f32(0.3) = 34.5000014: 35 wide (34 with the double 0.3)
    (40, 44, 0.8, 1),      # 40 * f32(0.8) = 32.0000005: the level exists
    (200, 200, 0.16, 0),   # 200 * f32(0.16) = 31.9999993: no level (32.0 with the double 0.16)
    (83, 70, 0.8, 3),      # 83 * 0.8^3 = 42.496
    (1600, 1600, 0.02, 0), # 1600 * f32(0.02) = 31.9999993: no level
])
def test_scale_table_depth_and_saturation(gpu_ctx, w, h, pyr_scale, depth):
    """the library's scale table has the depth flow_ref.scales states for the float32 pyr_scale:
    num_levels = 9 gives the bits of num_levels = depth, and one level fewer gives other bits"""
    assert len(R.scales(w, h, 9, R.f32(pyr_scale))) == depth + 1
    a, b = FC.frames("zoom", 81, w, h)
    run = lambda n: morph.optical_flow(gpu_ctx, a, b, morph.FlowParams(num_levels=n, num_iters=2, pyr_scale=pyr_scale))[0]
    full, sat = run(depth), run(9)
    assert np.array_equal(_bits(full), _bits(sat))
    assert np.array_equal(_bits(full), _bits(run(depth + 1)))
    if depth > 0:
        assert not np.array_equal(_bits(full), _bits(run(depth - 1)))


# ---- colour -------------------------------------------------------------------------------------

# one iteration at d = 0: no sample position is near a threshold, so nothing is excused (an integer
# shift on a smooth texture converges to x + d = w - 1 along a whole column)
COLOUR_KW = dict(num_levels=0, num_iters=1)


def _boundary_palette():
    """RGB triples whose weighted sum lands on the rounding boundary of (.. + 8192) >> 14: the sum is
    8192 mod 16384 (exactly .5, rounds up) or 8191 mod 16384 (just below, rounds down)"""
    r, g, b = np.mgrid[0:256, 0:256, 0:256]
    s = (4899 * r + 9617 * g + 1868 * b) % 16384
    up, down = np.argwhere(s == 8192), np.argwhere(s == 8191)
    assert len(up) > 100 and len(down) > 100
    return up.astype(np.uint8), down.astype(np.uint8)


def _boundary_frames(seed, w, h):
    rng = np.random.default_rng(seed)
    up, down = _boundary_palette()
    pal = np.concatenate([up, down])
    # sort the palette by grey so that a smooth index image gives a smooth, textured grey image
    pal = pal[np.argsort(R.grey(pal[None])[0], kind="stable")]
    t = R.blur(rng.random((h, w)), R.gauss_taps(1.0, 3))
    idx = np.rint((len(pal) - 1) * (t - t.min()) / (t.max() - t.min())).astype(np.int64)
    a = pal[idx]
    return np.ascontiguousarray(a), np.ascontiguousarray(np.roll(a, (1, 2), (0, 1)))


def _rgb_reference(a, b, kw):
    p = FC.spec_params(kw)
    d64, mask = R.flow(a, b, p, excuse=True)
    return d64, mask, R.flow(a, b, p, np.float32)


@pytest.mark.parametrize("kind", ["rgb", "red", "blue", "boundary"])
def test_rgb_entry_against_the_spec(gpu_ctx, kind):
    """independent R, G, B; one texture in R alone and in B alone; pixels on the rounding boundary"""
    w, h = 100, 70
    a, b = _boundary_frames(91, w, h) if kind == "boundary" else FC.rgb_frames(kind, 92, w, h)
    if kind == "boundary":
        c = a.astype(np.int64)
        s = (4899 * c[..., 0] + 9617 * c[..., 1] + 1868 * c[..., 2]) % 16384
        assert ((s == 8192) | (s == 8191)).all() and (s == 8192).any() and (s == 8191).any()
        assert np.ptp(R.grey(a)) > 100
    d64, mask, d32 = _rgb_reference(a, b, COLOUR_KW)
    got = morph.optical_flow(gpu_ctx, a, b, morph.FlowParams(**COLOUR_KW))[0]
    _check("rgb-" + kind, got, d64, d32, mask, 0.0)


def test_red_and_blue_textures_give_different_flows(gpu_ctx):
    """the same texture in R alone and in B alone: grey differs by the weights 4899 / 1868 only, and
    the flows differ (the 1e-3 regulariser of the solve does not scale with the image)"""
    w, h = 100, 70
    ar, br = FC.rgb_frames("red", 92, w, h)
    ab, bb = FC.rgb_frames("blue", 92, w, h)
    assert np.array_equal(ar[..., 0], ab[..., 2])
    fr = morph.optical_flow(gpu_ctx, ar, br, morph.FlowParams(**COLOUR_KW))[0]
    fb = morph.optical_flow(gpu_ctx, ab, bb, morph.FlowParams(**COLOUR_KW))[0]
    p = FC.spec_params(COLOUR_KW)
    want = np.abs(R.flow(ar, br, p) - R.flow(ab, bb, p)).max()
    print("red against blue: GPU %.3g px, spec %.3g px" % (np.abs(fr - fb).max(), want))
    assert want > 1e-2  # the spec tells them apart by far more than any tolerance here
    assert np.abs(fr - fb).max() > 0.5 * want


def _colour_videos(w, h, d):
    """two videos with independent R, G, B, each frame the base moved on by a few px"""
    base0, _ = FC.rgb_frames("rgb", 94, w, h)
    base1, _ = FC.rgb_frames("rgb", 95, w, h)
    v0 = np.stack([np.roll(base0, (t, 2 * t), (0, 1)) for t in range(d)])
    v1 = np.stack([np.roll(base1, (-t, t), (0, 1)) for t in range(d)])
    assert (v0[..., 0] != v0[..., 2]).mean() > 0.9 and (v1[..., 0] != v1[..., 2]).mean() > 0.9
    return v0, v1


def test_tracker_flows_on_colour_frames(gpu_ctx):
    """k_grey_rgba (the RGBA frames the tracker holds) on frames with independent R, G, B: the tracker's
    device-computed flows carry the bits of optical_flow on the RGB frames, which
    test_rgb_entry_against_the_spec pins to the spec"""
    w, h, d = 96, 64, 4
    v = _colour_videos(w, h, d)
    tr = morph.PointTracker(gpu_ctx, v[0], v[1])
    for k in range(2):
        fw = morph.optical_flow(gpu_ctx, v[k][:-1], v[k][1:])
        bw = morph.optical_flow(gpu_ctx, v[k][1:], v[k][:-1])
        assert np.abs(fw).max() > 0.5
        # the weights matter on these frames: with R and B swapped the flow is another one, by far more than the
        # float32 rounding of a default chain (below 1e-5 px in every default-parameter case of this module)
        swapped = morph.optical_flow(gpu_ctx, np.ascontiguousarray(v[k][:1, ..., ::-1]), np.ascontiguousarray(v[k][1:2, ..., ::-1]))
        assert np.abs(swapped[0] - fw[0]).max() > 1e-3
        for t in range(d):
            f, b = tr.get_flows(k, t)
            want_f = fw[t] if t < d - 1 else np.zeros_like(f)
            want_b = bw[t - 1] if t > 0 else np.zeros_like(b)
            assert np.array_equal(_bits(f), _bits(want_f)), (k, t)
            assert np.array_equal(_bits(b), _bits(want_b)), (k, t)


def test_sync_compute_flows_on_colour_frames(gpu_ctx):
    """the sync stage's k_grey_rgba call on the same videos.  The render reads a flow only where the
    field's Z is fractional (at an integer time the sample the flow positions has weight 0), so level 1
    gets Z = 0.5; then the pyramid that computed its flows renders the bytes of the one that was given
    optical_flow's, and not those of one with zero flows"""
    w, h, d = 96, 64, 4
    v0, v1 = _colour_videos(w, h, d)
    zero = np.zeros((d, h, w, 2), np.float32)
    f0, f1, _, _ = morph.video_optical_flows(gpu_ctx, v0, v1)
    assert np.abs(f0).max() > 0.5 and np.abs(f1).max() > 0.5
    up, comp, none = (morph.SyncPyramid(gpu_ctx) for _ in range(3))
    up.build(v0, v1, f0, f1, 16)
    comp.build(v0, v1, zero, zero, 16)
    none.build(v0, v1, zero, zero, 16)
    comp.compute_flows()
    assert len(up.levels) >= 2
    w1, h1, d1 = up.levels[1]
    field = [np.zeros((d1, h1, w1), np.float32), np.zeros((d1, h1, w1), np.float32), np.full((d1, h1, w1), 0.5, np.float32)]
    for p in (up, comp, none):
        p.set_field(1, *field)
    differ = 0
    for fa, frame in ((0.5, 1), (0.25, 2), (0.75, 0), (0.5, 2)):
        want = up.render_resample(fa, frame)
        assert np.array_equal(want, comp.render_resample(fa, frame)), (fa, frame)
        differ += int((want != none.render_resample(fa, frame)).sum())
    assert differ > 100, differ  # the flows reach the rendered bytes


# ---- arguments and host paths -------------------------------------------------------------------

def _call(gpu_ctx, fn, w, h, a_list, b_list, pitch, params=None):
    n = len(a_list)
    out = np.zeros((n, h, w, 2), np.float32)
    pa = (C.c_void_p * n)(*[x.ctypes.data for x in a_list])
    pb = (C.c_void_p * n)(*[x.ctypes.data for x in b_list])
    po = (C.c_void_p * n)(*[out[i].ctypes.data for i in range(n)])
    capi.check(fn(gpu_ctx._h, w, h, n, pa, pb, pitch, None if params is None else C.byref(params), po))
    return out


def test_pitch(gpu_ctx):
    """padded rows (NaN behind a luma row, 255 behind an RGB row) give the bits of the packed call"""
    w, h, pad = 65, 47, 7
    L = gpu_ctx._L
    a, b = FC.frames("noise", 96, w, h)
    packed = _call(gpu_ctx, L.vm_optical_flow_luma, w, h, [a], [b], 0)
    wide = [np.full((h, w + pad), np.nan, np.float32) for _ in range(2)]
    wide[0][:, :w], wide[1][:, :w] = a, b
    assert np.array_equal(_bits(_call(gpu_ctx, L.vm_optical_flow_luma, w, h, [wide[0]], [wide[1]], w + pad)), _bits(packed))
    assert np.array_equal(_bits(_call(gpu_ctx, L.vm_optical_flow_luma, w, h, [a], [b], w)), _bits(packed))
    assert np.isfinite(packed).all() and np.abs(packed).max() > 0.5
    ra, rb = FC.rgb_frames("rgb", 97, w, h)
    packed = _call(gpu_ctx, L.vm_optical_flow_rgb, w, h, [ra], [rb], 0)
    wide = [np.full((h, 3 * w + pad), 255, np.uint8) for _ in range(2)]   # a pitch that is no multiple of 3
    wide[0][:, :3 * w], wide[1][:, :3 * w] = ra.reshape(h, 3 * w), rb.reshape(h, 3 * w)
    assert np.array_equal(_bits(_call(gpu_ctx, L.vm_optical_flow_rgb, w, h, [wide[0]], [wide[1]], 3 * w + pad)), _bits(packed))
    for fn, x, y, pitch in ((L.vm_optical_flow_luma, a, b, w - 1), (L.vm_optical_flow_rgb, ra, rb, 3 * w - 1)):
        with pytest.raises(capi.VmError) as e:
            _call(gpu_ctx, fn, w, h, [x], [y], pitch)
        assert e.value.code == capi.VM_E_INVALID


def flow_pairs_per_chunk(w, h, p):
    """optical_flow_pairs' chunk: the pairs whose working set fits the 4 GiB budget (vm_flow.h)"""
    frame_bytes = sum(wk * hk * 20 for _, wk, hk in R.scales(w, h, p["num_levels"], p["pyr_scale"]))
    return int((4 << 30) / (2.0 * frame_bytes + w * h * 24))


def test_chunk_boundary_at_1080p(gpu_ctx):
    """more pairs than one chunk holds: the pairs on both sides of the boundary and the last one carry
    the bits of single-pair calls"""
    w, h = 1920, 1080
    per = flow_pairs_per_chunk(w, h, R.params())
    assert 20 <= per <= 32, per
    n = per + 2
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    base = (128 + 60 * np.sin(x / 7) * np.cos(y / 11) + 30 * np.sin((x + y) / 3)).astype(np.float32)
    fr = [np.ascontiguousarray(np.roll(base, (2 * t, 3 * t), (0, 1))) for t in range(5)]
    a_list = [fr[i % 5] for i in range(n)]
    b_list = [fr[(i + 1 + i // 5) % 5] for i in range(n)]
    L = gpu_ctx._L
    out = _call(gpu_ctx, L.vm_optical_flow_luma, w, h, a_list, b_list, 0)
    for i in (per - 1, per, n - 1):
        one = _call(gpu_ctx, L.vm_optical_flow_luma, w, h, [a_list[i]], [b_list[i]], 0)[0]
        assert np.array_equal(_bits(one), _bits(out[i])), i
        assert np.abs(one).max() > 0.5
    assert not np.array_equal(_bits(out[per - 1]), _bits(out[per]))
