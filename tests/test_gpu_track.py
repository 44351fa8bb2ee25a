"""The stage-2 point tracker on the GPU (vm_track.hip; MdiEditor::AddPoint / MovePoint / Histo,
UI/MdiEditor.cpp:1230-1393, 1516-1582) against its CPU statement (tests/track_ref.py): positions
identical and weights bit-identical on uploaded and on device-computed flows; segment independence;
the tracker's flows against vm_optical_flow_rgb and the stage-2 pyramid built from them; analytic
motion; NextStage's conversion end to end through a video solve."""
import ctypes as C

import numpy as np
import pytest

import track_ref as R
from test_gpu_flow import _rgb, _textured
from videomorphing_amd import capi, morph, synth

pytestmark = pytest.mark.gpu


def _video(rng, d, h, w):
    """few colours: shared bins, and pixels with 255 (uncounted)"""
    return (rng.integers(0, 6, (d, h, w, 3)) * 51).astype(np.uint8)


def _random_flows(rng, d, h, w):
    fl = [(rng.standard_normal((d, h, w, 2)) * 3).astype(np.float32) for _ in range(4)]
    for f in fl:
        f[rng.random((d, h, w)) < 0.15] = 0.5
        f[rng.random((d, h, w)) < 0.15] = -0.5
        f[rng.random((d, h, w)) < 0.05] = np.float32(np.nextafter(np.float32(0.5), np.float32(0)))
        f[rng.random((d, h, w)) < 0.03] = (40.0, -40.0)  # out of the frame
    return fl


def _random_segments(rng, n, d, h, w):
    segs = []
    for _ in range(n):
        side = int(rng.integers(0, 2))
        m = (int(rng.integers(-6, w + 6)), int(rng.integers(-6, h + 6)), int(rng.integers(0, d)))
        if rng.random() < 0.4:
            segs.append((side, ("chain", m, int(rng.choice([-1, 1])))))
        else:
            oz = int(rng.integers(0, d - 1))
            oz += oz >= m[2]
            o = (int(rng.integers(-6, w + 6)), int(rng.integers(-6, h + 6)), oz)
            segs.append((side, ("blend", m, o)))
    return segs


def _check(tracker, videos, flows, segs):
    """flows: (f0, f1, b0, b1); every covered frame identical to the spec, bit for bit"""
    out = tracker.propagate([morph._segment_tuple(side, s) for side, s in segs])
    d = tracker.depth
    n = 0
    for i, (side, s) in enumerate(segs):
        want = R.run_segment(videos[side], flows[side], flows[2 + side], s)
        assert sorted(want) == list(morph._covered(s, d))
        for t, (x, y, wt) in want.items():
            got = out[i, t]
            assert (int(got["x"]), int(got["y"])) == (x, y), (i, s, t)
            assert np.float32(got["weight"]).view(np.uint32) == np.float32(wt).view(np.uint32), (i, s, t, got["weight"], wt)
            n += 1
        for t in set(range(d)) - set(want):  # nothing else written
            assert out[i, t]["x"] == 0 and out[i, t]["y"] == 0 and out[i, t]["weight"] == 0
    return out, n


def test_matches_the_spec_on_uploaded_flows(gpu_ctx):
    rng = np.random.default_rng(11)
    d, h, w = 7, 40, 48
    videos = [_video(rng, d, h, w) for _ in range(2)]
    flows = _random_flows(rng, d, h, w)
    tr = morph.PointTracker(gpu_ctx, videos[0], videos[1], flows=flows)
    _, n = _check(tr, videos, flows, _random_segments(rng, 150, d, h, w))
    assert n > 300
    f, b = tr.get_flows(1, 3)
    assert np.array_equal(f, flows[1][3]) and np.array_equal(b, flows[3][3])


def test_matches_the_spec_on_computed_flows(gpu_ctx):
    rng = np.random.default_rng(12)
    d, h, w = 5, 64, 80
    videos = [np.stack([_rgb(_textured(w, h, t, s, 12.0)) for t in range(d)]) for s in ((1.5, -0.5), (-0.75, 1.25))]
    videos[0][:, 20:30, 20:30] = 255  # uncounted pixels
    tr = morph.PointTracker(gpu_ctx, videos[0], videos[1])
    got = [[tr.get_flows(k, t) for t in range(d)] for k in range(2)]
    flows = [np.stack([g[t][0] for t in range(d)]) for g in got] + [np.stack([g[t][1] for t in range(d)]) for g in got]
    assert not flows[0][-1].any() and not flows[2][0].any() and np.abs(flows[0][0]).max() > 0.5
    _check(tr, videos, flows, _random_segments(rng, 60, d, h, w))


def test_segments_do_not_depend_on_their_launch(gpu_ctx):
    rng = np.random.default_rng(13)
    d, h, w = 6, 36, 40
    videos = [_video(rng, d, h, w) for _ in range(2)]
    flows = _random_flows(rng, d, h, w)
    tr = morph.PointTracker(gpu_ctx, videos[0], videos[1], flows=flows)
    segs = [morph._segment_tuple(side, s) for side, s in _random_segments(rng, 120, d, h, w)]
    batch = tr.propagate(segs)
    for i in (0, 7, 63, 119):
        alone = tr.propagate([segs[i]])
        assert np.array_equal(alone[0].view(np.uint8), batch[i].view(np.uint8)), i
    assert {s[0] for s in segs} == {0, 1}


def test_compute_flows_equal_optical_flow_rgb(gpu_ctx):
    d, h, w = 4, 64, 96
    fr = [synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25)) for t in range(d)]
    v = [np.stack([_rgb(f[k]) for f in fr]) for k in range(2)]
    tr = morph.PointTracker(gpu_ctx, v[0], v[1])
    for k in range(2):
        fw = morph.optical_flow(gpu_ctx, v[k][:-1], v[k][1:])
        bw = morph.optical_flow(gpu_ctx, v[k][1:], v[k][:-1])
        for t in range(d):
            f, b = tr.get_flows(k, t)
            want_f = fw[t] if t < d - 1 else np.zeros_like(f)
            want_b = bw[t - 1] if t > 0 else np.zeros_like(b)
            assert np.array_equal(f.view(np.uint32), want_f.view(np.uint32)), (k, t)
            assert np.array_equal(b.view(np.uint32), want_b.view(np.uint32)), (k, t)


def test_video_pyramid_from_the_tracker(gpu_ctx):
    w, h, d = 96, 64, 5
    fr = [synth.make_video_pair(w, h, t, (0.5, 0.25), (1.5, -0.25)) for t in range(d)]
    rgb0, rgb1 = np.stack([_rgb(f[0]) for f in fr]), np.stack([_rgb(f[1]) for f in fr])
    levels, factor_t = synth.video_levels(w, h, d, 16)
    a, b = morph.VideoPyramid(gpu_ctx), morph.VideoPyramid(gpu_ctx)
    a.build_levels(levels, factor_t, d)
    b.build_levels(levels, factor_t, d)
    a.build_flows_rgb(rgb0, rgb1)
    tr = morph.PointTracker(gpu_ctx, rgb0, rgb1)
    b.build_flows_track(tr)
    for l in range(len(levels) - 1):
        for t in range(levels[l][2]):
            for name in ("f0", "f1", "b0", "b1"):
                x, y = a.pages[l][t].field(name), b.pages[l][t].field(name)
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), (l, t, name)
    small = morph.PointTracker(gpu_ctx, rgb0[:4], rgb1[:4])
    with pytest.raises(capi.VmError) as e:
        b.build_flows_track(small)
    assert e.value.code == capi.VM_E_INVALID


def test_points_follow_a_translating_video(gpu_ctx):
    d, h, w = 8, 96, 128
    shift = (2.0, -1.0)
    v = np.stack([_rgb(_textured(w, h, t, shift, 10.0)) for t in range(d)])
    tr = morph.PointTracker(gpu_ctx, v, v)
    P = morph.Parameters()
    starts = [(30, 60, 0), (50, 70, 3), (64, 48, 7), (40, 70, 5)]
    for x, y, z in starts:
        i = P.add_point(0, x, y, z, tr)
        for t in range(d):
            p = P.lp[i][t]
            assert p.p[:3] == (x + 2 * (t - z), y - (t - z), t), (x, y, z, t, p.p)
            assert p.p[3] == (1 if t == z else 0) and 0.0 <= p.weight <= 1.0 + 1e-6
    # a moved key in the middle: blends of two exact chains stay exact
    P.move_point(0, 0, 4, 38, 56, tr)
    assert all(P.lp[0][t].p[:2] == (30 + 2 * t, 60 - t) for t in range(d))


def test_stage_two_parameters_against_the_spec(gpu_ctx):
    rng = np.random.default_rng(14)
    d, h, w = 5, 64, 80
    s0, s1 = (0.5, 0.25), (1.5, -0.25)
    fr = [synth.make_video_pair(w, h, t, s0, s1) for t in range(d)]
    videos = [np.stack([_rgb(f[k]) for f in fr]) for k in range(2)]
    tr = morph.PointTracker(gpu_ctx, videos[0], videos[1])
    got = [[tr.get_flows(k, t) for t in range(d)] for k in range(2)]
    flows = [[np.stack([g[t][j] for t in range(d)]) for j in range(2)] for g in got]
    Ps = morph.Parameters()
    lp, rp, cnt = [], [], []
    for i in range(4):  # stage-1 tracks of one point each, connected in lists of 1..3
        lp.append([(int(rng.integers(8, w - 8)), int(rng.integers(8, h - 8)), int(rng.integers(0, d))) for _ in range(3)])
        rp.append([(int(rng.integers(8, w - 8)), int(rng.integers(8, h - 8)), int(rng.integers(0, d))) for _ in range(3)])
    for i in range(3):
        cnt.append([((i, j), (i + 1, j)) for j in range(i + 1)])
    Ps.lp = [[morph.Conp(*p) for p in t] for t in lp]
    Ps.rp = [[morph.Conp(*p) for p in t] for t in rp]
    Ps.cnt = [[morph.Connect(a, b) for a, b in row] for row in cnt]
    P2 = morph.stage_two_parameters(Ps, tr)
    L, Rr, cnt2 = R.next_stage(videos, flows, lp, rp, cnt)
    for mine, ref in ((P2.lp, L), (P2.rp, Rr)):
        assert len(mine) == len(ref) == 3
        for a, b in zip(mine, ref):
            for p, q in zip(a, b):
                assert p.p == tuple(q[:4]) and np.float32(p.weight).view(np.uint32) == np.float32(q[4]).view(np.uint32)
    assert [[(c.li, c.ri) for c in row] for row in P2.cnt] == cnt2
    # the stage-2 solve consumes them (min(weight_l, weight_r) per frame)
    cons = morph.video_constraints(P2)
    assert len(cons) == 3 * d and (cons[:, 4] <= 1).all()
    P2.max_iter, P2.max_iter_drop_factor, P2.start_res = 4, 1.0, 16
    vid = morph.VideoPyramid(gpu_ctx)
    levels, factor_t = synth.video_levels(w, h, d, 16)
    vid.build_levels(levels, factor_t, d)
    for t in range(d):
        vid.build_rgb_frame(t, videos[0][t], videos[1][t])
    vid.build_flows_track(tr)
    assert morph.VideoMorph(P2, vid).calculate_halfway_parametrization()
    assert np.isfinite(vid.pages[0][0].v).all()


def test_bad_segments_and_missing_data(gpu_ctx):
    d, h, w = 4, 40, 40
    z = np.zeros((d, h, w, 3), np.uint8)
    L = capi.load()
    h_ = C.c_void_p()
    capi.check(L.vm_track_create(gpu_ctx._h, w, h, d, C.byref(h_)))
    try:
        out = np.zeros((1, d), morph.TRACK_POINT)

        def run(*seg):
            arr = (capi.TrackSegment * 1)(capi.TrackSegment(*seg))
            return L.vm_track_propagate(h_, arr, 1, out.ctypes.data)

        for bad in ((2, 1, 1, 0, 0, 0, -1, 1), (0, 1, 1, 4, 0, 0, -1, 1), (0, 1, 1, 0, 0, 0, -1, 0),
                    (0, 1, 1, 1, 2, 2, 1, 0), (0, 1, 1, 1, 2, 2, 3, -1), (0, 1, 1, 1, 2, 2, 4, 0)):
            assert run(*bad) == capi.VM_E_INVALID, bad
        assert run(0, 1, 1, 0, 0, 0, -1, 1) == capi.VM_E_STATE  # no frames yet
        for t in range(d):
            capi.check(L.vm_track_upload_frame(h_, 0, t, z[t].ctypes.data, 0))
        assert run(0, 1, 1, 0, 0, 0, -1, 1) == capi.VM_E_STATE  # no flows yet
        assert run(0, 1, 1, 0, 0, 0, -1, -1) == capi.VM_OK  # a chain from frame 0 backwards covers nothing
        assert run(0, 1, 1, 1, 3, 3, 2, 0) == capi.VM_OK  # adjacent keys: nothing between, no flow read
        assert L.vm_track_compute_flows(h_, None) == capi.VM_E_STATE  # video 1 missing
        assert L.vm_track_upload_frame(h_, 0, d, z[0].ctypes.data, 0) == capi.VM_E_INVALID
        # flows that are not finite or beyond +-1e5 px, keys beyond +-1e6 px: every position must stay an int
        fl = np.zeros((h, w, 2), np.float32)
        for bad in (np.nan, np.inf, 1.5e5, -2e5):
            fl[7, 9, 1] = bad
            assert L.vm_track_upload_flows(h_, 0, 1, fl.ctypes.data, None, 0) == capi.VM_E_INVALID, bad
            assert L.vm_track_upload_flows(h_, 0, 1, None, fl.ctypes.data, 0) == capi.VM_E_INVALID, bad
        fl[7, 9, 1] = 1e5
        capi.check(L.vm_track_upload_flows(h_, 0, 1, fl.ctypes.data, fl.ctypes.data, 0))
        assert run(0, 2000001, 1, 1, 0, 0, -1, -1) == capi.VM_E_INVALID
        assert run(0, 1, 1, 1, 3, -1000001, 2, 0) == capi.VM_E_INVALID
        assert run(0, 1000000, -1000000, 1, 0, 0, -1, -1) == capi.VM_OK
        assert L.vm_track_create(gpu_ctx._h, w, h, 16385, C.byref(C.c_void_p())) == capi.VM_E_INVALID
        with pytest.raises(capi.VmError):
            morph.PointTracker(gpu_ctx, z[:, :20], z[:, :20])  # below 32 x 32
    finally:
        L.vm_track_destroy(h_)


def test_compute_flows_replace_uploaded_flags(gpu_ctx):
    """a failed vm_track_compute_flows leaves no flow counted as supplied"""
    d, h, w = 3, 40, 48
    v = np.full((d, h, w, 3), 100, np.uint8)
    tr = morph.PointTracker(gpu_ctx, v, v, flows=[np.zeros((d, h, w, 2), np.float32)] * 4)
    bad = capi.FlowParams()
    capi.load().vm_flow_params_default(C.byref(bad))
    bad.win_size = 12
    assert tr._L.vm_track_compute_flows(tr._h, C.byref(bad)) == capi.VM_E_INVALID  # rejected before any write
    assert tr.propagate([(0, 5, 5, 0, 0, 0, -1, 1)])[0, 2]["x"] == 5


def test_stage_two_rejects_an_empty_list(gpu_ctx):
    d, h, w = 3, 40, 48
    v = np.full((d, h, w, 3), 100, np.uint8)
    tr = morph.PointTracker(gpu_ctx, v, v, flows=[np.zeros((d, h, w, 2), np.float32)] * 4)
    Ps = morph.Parameters()
    Ps.add_point_pair(5, 5, 6, 6)
    Ps.cnt.append([])
    with pytest.raises(ValueError):
        morph.stage_two_parameters(Ps, tr)


def test_tracker_destroyed_after_its_context(vmlib):
    ctx = morph.Context(0)
    d, h, w = 3, 40, 48
    v = np.full((d, h, w, 3), 100, np.uint8)
    tr = morph.PointTracker(ctx, v, v, flows=[np.zeros((d, h, w, 2), np.float32)] * 4)
    assert tr.propagate([(0, 5, 5, 0, 0, 0, -1, 1)])[0, 2]["x"] == 5  # 5 + (0 + 0.5) truncates to 5
    ctx.close()
    with pytest.raises(capi.VmError):
        tr.propagate([(0, 5, 5, 0, 0, 0, -1, 1)])
    tr.close()
