"""The temporal coherence path on the GPU against the oracle: the flow
splat / initialize_temp / temporal upsample kernels bit for bit (the 64-bit fixed-point
accumulation is order-independent), the flag == true energy term bit for bit in EXACT mode under
every sweep schedule, whole video solves incl. the middle-page-outward chain bit for bit, FAST
within its stated tolerance, and the device-side flow pyramid against the oracle's restatement
of Pyramid::build's flow half.

Each stage here runs at one shape on smooth flows.  The stages at their edges (whole-number and
colliding landings, holes, rows without weight, footprints cut by the frame, level sizes around the
64-wide workgroup), the term under every schedule on drawn levels (w_temp, factor_d, masks,
constraints, boundary conditions) and a pyramid whose second level is the largest are
tests/test_gpu_temporal_stages.py; the oracle itself is held to a numpy statement of upsample.cu
by tests/test_temporal_ref.py (tests/temporal_ref.py, tests/temporal_cases.py)."""
import ctypes as C

import numpy as np
import pytest

from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu


def _smooth_flow(rng, w, h, amp):
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    a, b, c, d = rng.rand(4) * 2 * np.pi
    fx = amp * np.sin(2 * np.pi * x / w + a) * np.cos(2 * np.pi * y / h + b) + 0.3 * amp
    fy = amp * np.cos(2 * np.pi * x / w + c) * np.sin(2 * np.pi * y / h + d) - 0.2 * amp
    return np.stack([fx, fy], -1).astype(np.float32)


def _make(O, ctx, levels, factor_t=None, depth0=None, seed=0, flow_amp=1.2, noise=3.0):
    """the same synthetic video in the oracle and on the device: per page lumas (the pair of
    synth.make_pair + per-frame noise, box-filtered per level) and four smooth flow fields"""
    rng = np.random.RandomState(seed)
    w0, h0, d0 = levels[0]
    vid = O.Video(levels, depth0)
    dev = morph.VideoPyramid(ctx)
    dev.build_levels(levels, factor_t, depth0)
    ft = dev.factor_t
    frames = synth.page_frames(levels, ft)
    base = [synth.make_pair(w0, h0, frame=t, amp=0.012 * w0) for t in range(d0)]
    base = [(a + noise * rng.randn(h0, w0).astype(np.float32), b + noise * rng.randn(h0, w0).astype(np.float32)) for a, b in base]
    pyrs = [synth.build_pyramid(a, b, len(levels)) for a, b in base]
    for l, (w, h, d) in enumerate(levels[:-1]):
        fl = {k: [_smooth_flow(rng, w, h, flow_amp * w / w0) for _ in range(d)] for k in ("f0", "f1", "b0", "b1")}
        vid.set_flows(l, fl)
        for t in range(d):
            i0, i1 = pyrs[frames[l][t]][l]
            vid.set_images(l, t, i0, i1)
            dev.upload_luma(l, t, i0, i1)
            dev.upload_flows(l, t, fl["f0"][t], fl["f1"][t], fl["b0"][t], fl["b1"][t])
    return vid, dev


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _kp(ctx, O, **kw):
    P = O.default_params(**kw)
    kp = capi.KernParams()
    for f, _ in capi.KernParams._fields_:
        setattr(kp, f, getattr(P, f))
    ctx.set_params(kp)
    return P


def test_initialize_temp_exact(gpu_ctx, oracle):
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle)
    levels = [(53, 37, 3), (27, 19, 3)]
    vid, dev = _make(oracle, gpu_ctx, levels, seed=3)
    rng = np.random.RandomState(7)
    L = dev._L
    for t in range(3):
        v = (rng.randn(37, 53, 2) * 1.5).astype(np.float32)
        vid.pages[0][t].field("v")[...] = v
        dev.pages[0][t].v = v
    vid.init_level(0, P)
    capi.check(L.vm_video_init_level(dev._h, 0, None, 0))
    for page, dr in ((2, -1), (0, +1)):
        src = page + dr
        fl = vid.flows[0]
        fa, fb = (fl["f0"][src], fl["f1"][src]) if dr < 0 else (fl["b0"][src], fl["b1"][src])
        vid.pages[0][page].initialize_temp(vid.pages[0][src], fa, fb)
        capi.check(L.vm_video_initialize_temp(dev._h, 0, page, dr))
        ref_o, mask_o = vid.pages[0][page].field("temp_ref"), vid.pages[0][page].field("temp_mask")
        assert np.array_equal(_bits(mask_o), _bits(dev.pages[0][page].field("temp_mask")))
        assert np.array_equal(_bits(ref_o), _bits(dev.pages[0][page].field("temp_ref")))
        assert (mask_o > 0).mean() > 0.8 and (mask_o == 0).any()      # holes where nothing landed
    with pytest.raises(capi.VmError):
        capi.check(L.vm_video_initialize_temp(dev._h, 0, 0, -1))     # page 0 has no predecessor


def test_video_upsample_with_depth_doubling_exact(gpu_ctx, oracle):
    """upsample(): 3 coarse pages -> 5 fine pages; pages 1 and 3 are splatted from their two
    neighbours along the flows, smoothed and row-filled (upsample.cu:297-338)"""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    _kp(gpu_ctx, oracle)
    levels = [(46, 34, 5), (23, 17, 3)]
    vid, dev = _make(oracle, gpu_ctx, levels, factor_t=[1, 2], seed=5, flow_amp=4.0)
    rng = np.random.RandomState(9)
    for t in range(3):
        v = (rng.randn(17, 23, 2) * 0.8).astype(np.float32)
        vid.pages[1][t].field("v")[...] = v
        dev.pages[1][t].v = v
    vid.upsample(0)
    capi.check(dev._L.vm_video_upsample(dev._h, 0))
    for t in range(5):
        a, b = vid.pages[0][t].field("v"), dev.pages[0][t].v
        assert np.array_equal(_bits(a), _bits(b)), (t, np.abs(a - b).max())
    assert np.abs(vid.pages[0][1].field("v")).max() > 0.1
    # even depths: the last odd page stays zero (upsample.cu:307-308 skips i == depth-1)
    levels = [(46, 34, 4), (23, 17, 2)]
    vid, dev = _make(oracle, gpu_ctx, levels, factor_t=[1, 2], seed=6)
    for t in range(2):
        v = (rng.randn(17, 23, 2) * 0.8).astype(np.float32)
        vid.pages[1][t].field("v")[...] = v
        dev.pages[1][t].v = v
    vid.upsample(0)
    capi.check(dev._L.vm_video_upsample(dev._h, 0))
    for t in range(4):
        assert np.array_equal(_bits(vid.pages[0][t].field("v")), _bits(dev.pages[0][t].v)), t
    assert not dev.pages[0][3].v.any() and dev.pages[0][2].v.any()


@pytest.mark.parametrize("sched", [capi.SWEEP_TILE, capi.SWEEP_SPLIT, capi.SWEEP_STEP, capi.SWEEP_PASS])
def test_sweeps_with_the_temporal_term_exact(gpu_ctx, oracle, sched):
    """flag == true in every schedule: one page tied to its neighbour, 3 iterations, bit-identical"""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle, w_temp=25.0)
    levels = [(90, 50, 2), (45, 25, 2)]
    vid, dev = _make(oracle, gpu_ctx, levels, seed=11)
    rng = np.random.RandomState(13)
    L = dev._L
    try:
        gpu_ctx.set_tuning(sched, 0, 0)
        for t in range(2):
            v = (0.7 * synth.displacement(90, 50, amp=1.0) + 0.1 * rng.randn(50, 90, 2)).astype(np.float32)
            vid.pages[0][t].field("v")[...] = v
            dev.pages[0][t].v = v
        vid.init_level(0, P)
        capi.check(L.vm_video_init_level(dev._h, 0, None, 0))
        its = vid.optimize_level(0, P, 3)
        prog = (capi.Progress * 2)()
        capi.check(L.vm_video_optimize_level(dev._h, 0, 3.0, None, 0, prog))
    finally:
        gpu_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
    assert [prog[t].iters for t in range(2)] == [its[0], its[1]]
    for t in range(2):
        for f in ("v", "mean", "var", "cross", "value", "tps_b", "luma"):
            assert np.array_equal(_bits(vid.pages[0][t].field(f)), _bits(dev.pages[0][t].field(f))), (t, f)
    # the term did something: page 0 (tied to page 1) differs from an untied solve
    assert vid.pages[0][0].field("temp_mask").max() > 0


@pytest.mark.parametrize("resident", [0, 2, 3])
def test_sparse_sweeps_with_the_temporal_term_fast(gpu_ctx, oracle, resident):
    """flag == true, FAST, a long run into the pruned regime: the SPARSE schedule (its lean kernel reads the temporal
    reference and weight beside the LDS copy of the pixel's own state; resident visits automatic / re-centred at every
    commit / given up at the first) ends bit-identical to the TILE schedule, both pages"""
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    _kp(gpu_ctx, oracle, w_temp=25.0)
    levels = [(210, 118, 2), (105, 59, 2)]
    rng = np.random.RandomState(17)
    v0 = [(0.7 * synth.displacement(210, 118, amp=1.0) + 0.1 * rng.randn(118, 210, 2)).astype(np.float32) for t in range(2)]
    out = {}
    try:
        for sched in (capi.SWEEP_TILE, capi.SWEEP_SPARSE):
            vid, dev = _make(oracle, gpu_ctx, levels, seed=11)
            gpu_ctx.set_tuning(sched, 0, 0)
            gpu_ctx.set_sparse_resident(resident)
            for t in range(2):
                dev.pages[0][t].v = v0[t]
            capi.check(dev._L.vm_video_init_level(dev._h, 0, None, 0))
            prog = (capi.Progress * 2)()
            capi.check(dev._L.vm_video_optimize_level(dev._h, 0, 160.0, None, 1, prog))
            out[sched] = ([[dev.pages[0][t].field(f) for f in ("v", "mean", "var", "cross", "value", "tps_b", "luma")] for t in range(2)],
                          [(prog[t].iters, prog[t].commits, prog[t].candidates, prog[t].active_tiles) for t in range(2)])
    finally:
        gpu_ctx.set_tuning(capi.SWEEP_AUTO, 0, 0)
        gpu_ctx.set_sparse_resident(0)
        gpu_ctx.set_math_mode(capi.MATH_EXACT)
    assert out[capi.SWEEP_TILE][1] == out[capi.SWEEP_SPARSE][1], (out[capi.SWEEP_TILE][1], out[capi.SWEEP_SPARSE][1])
    assert out[capi.SWEEP_TILE][1][0][1] > 1000
    for t in range(2):
        for a, b in zip(out[capi.SWEEP_TILE][0][t], out[capi.SWEEP_SPARSE][0][t]):
            assert np.array_equal(_bits(a), _bits(b)), t


def test_video_solve_exact(gpu_ctx, oracle):
    """Morph::calculate_halfway_parametrization over a temporal pyramid (5 -> 3 pages), with
    point constraints on two frames and a locked border: level by level and in one
    vm_video_solve, bit-identical to the oracle incl. per-page iteration counts"""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle, w_temp=10.0, bcond=capi.BCOND_BORDER)
    levels = [(64, 48, 5), (32, 24, 5), (16, 12, 3)]
    ft = [1, 1, 2]
    vid, dev = _make(oracle, gpu_ctx, levels, factor_t=ft, seed=21)
    cons = np.float32([[20, 14, 23, 15, 1.0, 0], [40, 30, 38, 31, 0.7, 0], [22, 15, 25, 16, 1.0, 2],
                       [41, 29, 39, 30, 1.0, 4], [10, 40, 12, 41, 0.5, 3]])
    carr, n = morph._vcons_array(cons)
    L = dev._L
    # the coarse solve is a host solve on both sides (double, banded Cholesky): close, not bitwise;
    # the trajectory test starts both from the device's coarse solution
    vid.coarse_solve(P, cons)
    capi.check(L.vm_video_coarse_solve(dev._h, carr, n))
    for t in range(3):
        a, b = vid.pages[2][t].field("v"), dev.pages[2][t].v
        assert np.abs(a - b).max() < 1e-4 and (t != 1 or np.abs(b).max() > 0.1)   # coarse page 1 shows frame 2
        vid.pages[2][t].field("v")[...] = b
    mi = 6.0
    for el in (1, 0):
        vid.upsample(el)
        vid.init_level(el, P, cons)
        its = vid.optimize_level(el, P, mi)
        capi.check(L.vm_video_upsample(dev._h, el))
        capi.check(L.vm_video_init_level(dev._h, el, carr, n))
        prog = (capi.Progress * levels[el][2])()
        capi.check(L.vm_video_optimize_level(dev._h, el, mi, None, 0, prog))
        assert [prog[t].iters for t in range(levels[el][2])] == [its[t] for t in range(levels[el][2])]
        for t in range(levels[el][2]):
            for f in ("v", "ui_b", "tps_b", "value"):
                assert np.array_equal(_bits(vid.pages[el][t].field(f)), _bits(dev.pages[el][t].field(f))), (el, t, f)
    final = [dev.pages[0][t].v for t in range(5)]
    assert max(np.abs(v).max() for v in final) > 0.3
    # the one-call driver walks the same trajectory
    prog = (capi.Progress * 10)()
    capi.check(L.vm_video_solve(dev._h, 6.0, 1.0, carr, n, None, 0, prog))
    for t in range(5):
        assert np.array_equal(_bits(final[t]), _bits(dev.pages[0][t].v)), t
    assert prog[2].iters >= 1 and prog[2].elapsed_ms > 0


def test_video_solve_level_pipeline_exact(gpu_ctx, oracle):
    """levels that hold the same frames are pipelined by vm_video_solve (page p of level l starts as
    soon as page p of level l + 1 and its chain neighbour on level l are done, on parallel lanes):
    bit-identical to the oracle's level-by-level walk and to the driver with the pipeline off"""
    import os
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle, w_temp=10.0)
    levels = [(96, 64, 5), (48, 32, 5), (24, 16, 5), (12, 8, 5)]
    vid, dev = _make(oracle, gpu_ctx, levels, seed=33)
    cons = np.float32([[30, 20, 33, 21, 1.0, 0], [60, 40, 58, 41, 1.0, 2], [20, 50, 22, 48, 0.8, 4]])
    carr, n = morph._vcons_array(cons)
    L = dev._L
    capi.check(L.vm_video_coarse_solve(dev._h, carr, n))
    coarse = [dev.pages[3][t].v.copy() for t in range(5)]
    # the oracle, level by level, from the device's coarse solution
    for t in range(5):
        vid.pages[3][t].field("v")[...] = coarse[t]
    for el in (2, 1, 0):
        vid.upsample(el)
        vid.init_level(el, P, cons)
        vid.optimize_level(el, P, 8.0)
    results = {}
    for mode in ("pipeline", "sequential"):
        if mode == "sequential":
            os.environ["VM_NO_VIDEO_PIPELINE"] = "1"
        try:
            prog = (capi.Progress * 15)()
            capi.check(L.vm_video_solve(dev._h, 8.0, 1.0, carr, n, None, 0, prog))
        finally:
            os.environ.pop("VM_NO_VIDEO_PIPELINE", None)
        results[mode] = ([[dev.pages[el][t].v.copy() for t in range(5)] for el in range(3)], [prog[k].iters for k in range(15)])
    for el in range(3):
        for t in range(5):
            assert np.array_equal(_bits(results["pipeline"][0][el][t]), _bits(vid.pages[el][t].field("v"))), (el, t)
            assert np.array_equal(_bits(results["pipeline"][0][el][t]), _bits(results["sequential"][0][el][t])), (el, t)
    assert results["pipeline"][1] == results["sequential"][1] and min(results["pipeline"][1]) >= 1
    assert max(np.abs(v).max() for v in results["pipeline"][0][0]) > 0.2


def test_video_solve_fast_tolerance(gpu_ctx, oracle):
    """FAST arithmetic over a coupled video solve: the tolerance of the frame-pair path
    (tests/test_gpu_parity.py: RMS <= 0.05 px, >= 99 % of pixels within 0.25 px) per page"""
    _kp(gpu_ctx, oracle, w_temp=10.0)
    levels = [(96, 64, 3), (48, 32, 3), (24, 16, 3)]
    res = {}
    for mode in (capi.MATH_EXACT, capi.MATH_FAST):
        gpu_ctx.set_math_mode(mode)
        vid, dev = _make(oracle, gpu_ctx, levels, seed=31, noise=1.0)
        prog = (capi.Progress * 6)()
        capi.check(dev._L.vm_video_solve(dev._h, 30.0, 1.0, None, 0, None, 0, prog))
        res[mode] = [dev.pages[0][t].v for t in range(3)]
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    for t in range(3):
        dv = np.sqrt(((res[capi.MATH_EXACT][t] - res[capi.MATH_FAST][t]) ** 2).sum(-1))
        assert np.sqrt((dv ** 2).mean()) <= 0.05, (t, np.sqrt((dv ** 2).mean()))
        assert (dv < 0.25).mean() >= 0.99, (t, (dv < 0.25).mean())
    assert np.abs(res[capi.MATH_FAST][1]).max() > 0.3


def test_device_flow_pyramid_matches_the_oracle(gpu_ctx, oracle):
    """vm_video_build_flows (load(-50, 50) -> scale -> store -> x ratio -> temporal concatenation,
    pyramid.cu:284-326, 375-456) against the oracle's restatement, which is pinned by the
    reference's own resample library (tests/golden/flow_ref.npz)"""
    w, h, d, sr = 80, 64, 32, 8
    levels, ft = synth.video_levels(w, h, d, sr)
    assert [l[2] for l in levels] == [32, 32, 17, 9] and ft == [1, 1, 2, 2]   # level 2: flows of 17 pages, concatenated
    rng = np.random.RandomState(41)
    fam = [[_smooth_flow(rng, w, h, 2.0) for _ in range(d)] for _ in range(4)]
    want = oracle.flow_pyramids(fam[0], fam[1], fam[2], fam[3], levels, ft)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, ft, d)
    dev.build_flows(*fam)
    worst = 0.0
    for l in range(len(levels) - 1):
        for t in range(levels[l][2]):
            for k in ("f0", "f1", "b0", "b1"):
                worst = max(worst, np.abs(dev.pages[l][t].field(k) - want[l][k][t]).max())
    # px.  The derived bound of tests/test_gpu_pyramid_stages.py where it is the smaller one: with D = max |oracle -
    # float64 statement| the device stays within 4 D of float64, hence within 5 D of the oracle
    import pyramid_ref as R
    f64 = R.flow_pyramids(fam[0], fam[1], fam[2], fam[3], levels, ft)
    D = max(np.abs(np.stack(want[l][k]) - np.stack(f64[l][k])).max() for l in range(len(levels) - 1) for k in ("f0", "f1", "b0", "b1"))
    assert worst <= min(5e-3, 5 * D), (worst, D)
    # the flows of the halved level span two frames: about twice a plain rescale of one frame's flow
    one = oracle.flow_scale(want[1]["f0"][0], levels[2][0], levels[2][1])
    assert np.abs(want[2]["f0"][0]).mean() > 1.5 * np.abs(one).mean()


def test_device_video_luma_pyramid_pages(gpu_ctx, oracle):
    """vm_video_build_rgb: a frame's luma pyramid lands in every page that shows the frame"""
    w, h, d, sr = 80, 64, 32, 8
    levels, ft = synth.video_levels(w, h, d, sr)       # depths 32, 32, 17, 9 (the last: v only)
    frames = synth.page_frames(levels, ft)
    assert frames[2][4] == 8 and frames[2][16] == 31
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, ft, d)
    rgbs = [synth.make_rgb_pair(w, h, frame=t) for t in range(d)]
    for t in range(d):
        dev.build_rgb_frame(t, *rgbs[t])
    for l, t in ((0, 3), (1, 31), (2, 4), (2, 16)):
        f = frames[l][t]
        # the derived bound of tests/test_gpu_pyramid_stages.py where it is the smaller one: 5 D, D = max |oracle - float64|
        import pyramid_ref as R
        for k, name in enumerate(("img0", "img1")):
            want, f64 = oracle.luma_pyramid(rgbs[f][k], l + 1), R.luma_pyramid(rgbs[f][k], l + 1)
            D = max(np.abs(a - b).max() for a, b in zip(want, f64))
            assert np.abs(dev.pages[l][t].field(name) - want[l]).max() <= min(2e-2, 5 * D), (l, t, name, D)


def test_temporal_video_at_1080p(gpu_ctx):
    """full size, FAST: a 3-frame 1080p video pair (6 levels) with the synthetic videos' analytic
    flows (video 1 moves faster than video 0, so the halfway field changes from frame to frame),
    12 sweeps per level.  Checked through properties: every page of every level was swept; the
    outer pages carry a temporal reference covering (nearly) the whole frame, and that reference
    is the middle page's solution moved along the flows; the window sums of a tied page still
    equal their definition after all its commits; the coupled pages stay closer to their
    neighbour than pages solved without the term"""
    import test_gpu_fullsize as F
    w, h, d = 1920, 1080, 3
    s0, s1 = (0.5, 0.25), (1.5, -0.25)
    frames = [synth.make_video_pair(w, h, t, s0, s1) for t in range(d)]
    f0, f1, b0, b1 = synth.constant_flows(w, h, d, s0, s1)
    gpu_ctx.set_math_mode(capi.MATH_FAST)
    res = {}
    try:
        for wt in (10.0, 0.0):
            prm = morph.Parameters()
            prm.max_iter, prm.max_iter_drop_factor, prm.start_res, prm.w_temp = 12, 1.0, 32, wt
            vid = morph.VideoPyramid(gpu_ctx)
            vid.build(frames and [f[0] for f in frames], [f[1] for f in frames], f0, f1, b0, b1, 32)
            assert [l[2] for l in vid.levels] == [3] * 6
            vm = morph.VideoMorph(prm, vid)
            vm.calculate_halfway_parametrization()
            assert all(vm.progress[(l, t)]["iters"] >= 1 for l in range(5) for t in range(3))
            res[wt] = [vid.pages[0][t].v for t in range(d)]
            if wt > 0:
                mask, ref = vid.pages[0][2].field("temp_mask"), vid.pages[0][2].field("temp_ref")
                assert (mask > 0).mean() > 0.99
                # page 2's reference = page 1's v advected by the mean flow (1, 0) and changed by
                # (f1 - f0) / 2 = (0.5, -0.25): compare away from the border
                v1 = res[wt][1]
                want = v1[8:-8, 7:-9] + np.float32([0.5, -0.25])
                assert np.abs(ref[8:-8, 8:-8] - want).max() < 1e-3
                F._window_sum_invariants(vid.pages[0][2], frames[2][0], frames[2][1])
            del vid
    finally:
        gpu_ctx.set_math_mode(capi.MATH_EXACT)
    # the true field changes by (0.5, -0.25) per frame; with the term the pages follow their
    # advected neighbour more closely than when every frame is solved on its own
    dev = lambda r: np.abs((r[2][8:-8, 8:-8] - np.float32([0.5, -0.25])) - r[1][8:-8, 7:-9]).mean()
    assert dev(res[10.0]) < dev(res[0.0]), (dev(res[10.0]), dev(res[0.0]))


@pytest.mark.parametrize("levels,ft,depth0,full", [
    ([(64, 48, 5), (32, 24, 5), (16, 12, 3)], [1, 1, 2], 5, (64, 48)),
    ([(64, 48, 5), (32, 24, 5), (16, 12, 3)], [1, 1, 2], 5, (100, 75)),      # a decimated stage-2 pyramid: placeholder level larger
    ([(40, 30, 6), (20, 15, 4), (10, 8, 3)], [1, 2, 2], 6, (40, 30)),         # 6 -> 4 -> 3 pages: factors 4, 2; clamped last frame
    ([(40, 30, 4), (20, 15, 4)], [2, 1], 7, (40, 30)),                        # the finest level already skips frames (depth0 7 -> 4)
])
def test_video_result_delivery_exact(gpu_ctx, oracle, levels, ft, depth0, full):
    """CMatchingThread::update_result for depth > 1 (MatchingThread.cpp:22-84) from every level: page i
    scaled and resized into frame min(i * factor, depth0 - 1), the frames the temporal pyramid skipped
    blended from the frames around them -- all depth0 frames bit-identical to the oracle's restatement
    of the reference's two loops, as a host array and frame by frame in a device-resident vm_frame"""
    vid = oracle.Video(levels, depth0)
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, ft, depth0)
    rng = np.random.RandomState(17)
    for l, (w, h, d) in enumerate(levels):
        for t in range(d):
            v = (rng.randn(h, w, 2) * 1.5).astype(np.float32)
            vid.pages[l][t].field("v")[...] = v
            dev.pages[l][t].v = v
    w0, h0 = full
    fr = morph.Frame(gpu_ctx, w0, h0, 0)
    for l in range(len(levels)):
        ref = vid.update_result(l, w0, h0)
        got = dev.result(l, w0, h0)
        assert got.shape == (depth0, h0, w0, 2)
        for f in range(depth0):
            assert np.array_equal(_bits(ref[f]), _bits(got[f])), (l, f, np.abs(ref[f] - got[f]).max())
            fr.set_v_from_video(dev, l, f)
            assert np.array_equal(_bits(ref[f]), _bits(fr.download_v())), (l, f)
        factor = int(vid.factor_d[0] / vid.factor_d[l + 1])
        if factor > 1 and depth0 > 2:       # a skipped frame really is the blend of its neighbours
            assert np.allclose(got[1], got[0] * (1 - 1.0 / min(factor, depth0 - 1)) + got[min(factor, depth0 - 1)] / min(factor, depth0 - 1), atol=1e-5)
    fr.close()


def test_video_matching_thread_end_to_end(gpu_ctx, oracle):
    """The temporally coupled path to the screen: VideoMatchingThread (solve on a worker thread, then
    update_result) -> per frame the field into a device-resident vm_frame -> Poisson extension of
    both sides -> rendered halfway frame.  The delivered fields equal the oracle's solve + its
    restatement of update_result bit for bit (EXACT); the rendered frame of every video frame
    equals the oracle's renderer on the oracle's extension within the Poisson solver's +-1 level."""
    gpu_ctx.set_math_mode(capi.MATH_EXACT)
    P = _kp(gpu_ctx, oracle, w_temp=10.0)
    levels, ft = [(64, 48, 5), (32, 24, 5), (16, 12, 3)], [1, 1, 2]
    vid, dev = _make(oracle, gpu_ctx, levels, factor_t=ft, seed=31)
    vid.solve(P, 12, 1.0)
    prm = morph.Parameters()
    prm.max_iter, prm.max_iter_drop_factor = 12, 1.0
    th = morph.VideoMatchingThread(prm, dev)
    th.start()
    th.wait()
    ref = vid.update_result(0)
    assert len(dev._vector) == 5 and th.percentage == 100.0
    for f in range(5):
        assert np.array_equal(_bits(ref[f]), _bits(dev._vector[f])), f
    assert max(np.abs(r).max() for r in ref) > 0.2
    # compositor, frame by frame, v never leaving the device
    w, h = levels[0][:2]
    ex = int(0.1 * max(w, h))
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    fr = morph.Frame(gpu_ctx, w, h, ex)
    for f in (0, 2, 4):
        e0, e1 = morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex)
        fr.upload(e0, e1, None, None)
        fr.set_v_from_video(dev, 0, f)
        crops = {1: e1[ex:ex + h, ex:ex + w].copy(), 2: e0[ex:ex + h, ex:ex + w].copy()}
        for side, ext in ((1, e0), (2, e1)):
            r, _, _ = oracle.poisson_extend(ext, w, h, ex, crops[side], ref[f], side, tol=1e-9)
            fr.poisson_extend(side, tol=1e-6)
            ext[...] = r
        img = fr.render_halfway(0.5, 0.5, 1)
        want = oracle.render_halfway(w, h, ex, 0.5, 0.5, 1, e0.astype(np.float32), e1.astype(np.float32), ref[f], np.zeros_like(ref[f]))
        d = np.abs(img.astype(int) - want.astype(int))
        assert d.max() <= 1, (f, d.max())
    fr.close()


def test_video_result_at_1080p(gpu_ctx):
    """update_result at full size, through properties: from a level whose temporal stride is 2 (3 pages of
    960x540 for a 5-frame 1080p video) the key frames are exactly what the frame-pair path's
    vm_upscale_result makes of the same page, the skipped frames exactly the mean of their neighbours,
    and the device-resident vm_frame receives the same bits"""
    w0, h0 = 1920, 1080
    levels, ft = [(1920, 1080, 5), (960, 540, 3), (480, 270, 3)], [1, 2, 1]
    dev = morph.VideoPyramid(gpu_ctx)
    dev.build_levels(levels, ft, 5)
    rng = np.random.RandomState(5)
    pages = [(rng.randn(540, 960, 2) * 2).astype(np.float32) for _ in range(3)]
    for t in range(3):
        dev.pages[1][t].v = pages[t]
    got = dev.result(1)
    pyr = morph.Pyramid(gpu_ctx)
    pyr.build_levels([(w0, h0), (960, 540)])
    for t in range(3):
        pyr[2].v = pages[t]
        want = np.zeros((h0, w0, 2), np.float32)
        capi.check(pyr._L.vm_upscale_result(pyr._h, 1, w0, h0, want.ctypes.data, 0))
        assert np.array_equal(_bits(want), _bits(got[2 * t])), t
    half = np.float32(0.5)
    for f in (1, 3):
        assert np.array_equal(_bits(got[f - 1] * half + got[f + 1] * half), _bits(got[f])), f
    fr = morph.Frame(gpu_ctx, w0, h0, 0)
    for f in range(5):
        fr.set_v_from_video(dev, 1, f)
        assert np.array_equal(_bits(got[f]), _bits(fr.download_v())), f
    fr.close()
