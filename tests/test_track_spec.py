"""The stage-2 point tracker's spec (tests/track_ref.py) checked on the CPU: known answers
of the flow step and of Histo, the literal AddPoint / MovePoint sequence against the segment form the
kernel computes, NextStage's conversion, ConnectPoint's stage-2 branch, and the tracker C-ABI's
argument checks (no device is touched)."""
import ctypes as C

import numpy as np

import track_ref as R
from videomorphing_amd import capi, morph


def test_step_known_answers():
    assert R.step(10, 20, (0.6, 0.0)) == (11, 20)          # 10 + 1.1 -> 11
    assert R.step(3, 0, (0.0, -0.6)) == (3, 0)             # 0 - 0.1 truncates toward zero
    assert R.step(3, 5, (0.0, -0.6)) == (3, 4)             # 5 - 0.1 -> 4
    assert R.step(0, 0, (-0.4, 0.4)) == (0, 0)
    assert R.step(-2, 7, (-1.0, 0.0)) == (-2, 7)           # -2 - 0.5 -> -2
    flow = np.zeros((8, 10, 2), np.float32)
    flow[...] = (5.0, -4.0)
    x, y = 8, 2
    for _ in range(3):  # points leaving the frame are not clamped; the flow is read at the clamped point
        x, y = R.flow_step(x, y, flow)
    assert (x, y) == (23, -7)
    flow[0, 9] = (-30.0, 0.0)
    assert R.flow_step(40, -3, flow) == (10, -2)  # -3 + 0.5 -> -2


def test_bin_table():
    assert len(R.BIN) == 255 and R.BIN[0] == 0 and R.BIN[25] == 0 and R.BIN[26] == 1 and R.BIN[254] == 9
    assert R.BIN[51] == 2 and R.BIN[50] == 1


def _frame(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_histo_known_answers():
    fr = _frame(20, 24, 1)
    video = np.stack([fr, fr])
    assert R.histo(video, (10, 10, 0), (10, 10, 1)) == np.float32(1.0)  # identical patches
    # 255 in any channel: the pixel is not counted
    f2 = fr.copy()
    f2[7:13, 7:13, 1] = 255
    assert R.patch_hist(f2, 10, 10).sum() == 0
    f2[9, 9, 1] = 3
    assert R.patch_hist(f2, 10, 10).sum() == 1
    # border patches: rows [cl(y-3), cl(y+3)) -- 3 rows at y = 0, 6 inside, 3 at the last row, half-open
    for y, rows in ((0, 3), (1, 4), (2, 5), (3, 6), (10, 6), (18, 4), (19, 3)):
        assert R.patch_hist(np.full((20, 24, 3), 7, np.uint8), 10, y).sum() == rows * 6, y
    # beyond the frame: empty; an empty patch against anything gives 1.0
    for x, y in ((-4, 5), (30, 5), (5, -9), (5, 40)):
        assert R.patch_hist(fr, x, y).sum() == 0
        assert R.histo(video, (x, y, 0), (10, 10, 1)) == np.float32(1.0)


def test_histo_against_corrcoef():
    rng = np.random.default_rng(3)
    for _ in range(20):
        a = np.stack([_frame(16, 16, int(rng.integers(1 << 30))) // 32 * 32] * 2)  # few colours: overlapping bins
        p, q = tuple(int(v) for v in rng.integers(0, 16, 2)) + (0,), tuple(int(v) for v in rng.integers(0, 16, 2)) + (1,)
        h1, h2 = R.patch_hist(a[0], p[0], p[1]), R.patch_hist(a[1], q[0], q[1])
        want = abs(np.corrcoef(h1.astype(np.float64), h2.astype(np.float64))[0, 1])
        assert abs(float(R.histo(a, p, q)) - want) < 1e-6


def _random_case(rng):
    d = int(rng.integers(2, 14))
    h, w = int(rng.integers(8, 20)), int(rng.integers(8, 20))
    video = (rng.integers(0, 4, (d, h, w, 3)) * 85).astype(np.uint8)  # 0, 85, 170, 255: shared bins, some uncounted
    f = (rng.standard_normal((d, h, w, 2)) * 2.5).astype(np.float32)
    b = (rng.standard_normal((d, h, w, 2)) * 2.5).astype(np.float32)
    f[rng.random((d, h, w)) < 0.2] = 0.5  # exactly on the rounding edge
    b[rng.random((d, h, w)) < 0.2] = -0.5
    edits = [(int(rng.integers(-4, w + 4)), int(rng.integers(-4, h + 4)), int(rng.integers(0, d)))
             for _ in range(int(rng.integers(1, 6)))]
    return video, f, b, edits


def _same(a, b):
    return all(p[:4] == q[:4] and np.float32(p[4]).view(np.uint32) == np.float32(q[4]).view(np.uint32) for p, q in zip(a, b))


def test_sequential_edits_equal_the_segment_form():
    rng = np.random.default_rng(2024)
    blends = 0
    for case in range(220):
        video, f, b, edits = _random_case(rng)
        seq = R.edit_sequence(video, f, b, edits)
        seg = R.segment_track(video, f, b, edits)
        assert len(seq) == len(video) and _same(seq, seg), (case, edits)
        blends += sum(s[0] == "blend" for s in R.key_segments(R.final_keys(edits)))
    assert blends > 100


def test_next_stage_conversion():
    # stage-1 tracks (x, y, z) and two lists of connections
    lp = [[(10, 11, 0), (12, 13, 3)], [(20, 21, 5)]]
    rp = [[(30, 31, 1), (32, 33, 4)], [(40, 41, 2)]]
    cnt = [[((0, 0), (0, 0)), ((0, 1), (0, 1)), ((1, 0), (1, 0))], [((1, 0), (0, 1))]]
    le, re_ = R.next_stage_edits(lp, rp, cnt)
    assert le == [[(10, 11, 0), (12, 13, 3), (20, 21, 3)], [(20, 21, 4)]]
    assert re_ == [[(30, 31, 0), (32, 33, 3), (40, 41, 3)], [(32, 33, 4)]]
    rng = np.random.default_rng(5)
    d, h, w = 6, 14, 16
    videos = [(rng.integers(0, 4, (d, h, w, 3)) * 85).astype(np.uint8) for _ in range(2)]
    flows = [[(rng.standard_normal((d, h, w, 2)) * 2).astype(np.float32) for _ in range(2)] for _ in range(2)]
    L, Rr, cnt2 = R.next_stage(videos, flows, lp, rp, cnt)
    assert len(L) == len(Rr) == 2 and cnt2[1] == [((1, t), (1, t)) for t in range(d)]
    assert L[0][3][:4] == [20, 21, 3, 1] and L[0][0][:4] == [10, 11, 0, 1]  # the later key on frame 3 wins
    for k, tracks in enumerate((L, Rr)):
        for i, e in enumerate((le, re_)[k]):
            assert _same(tracks[i], R.segment_track(videos[k], flows[k][0], flows[k][1], e))


def test_connect_point_add_and_remove():
    P = morph.Parameters()
    d = 4
    for _ in range(3):
        P.lp.append([morph.Conp(0, 0, t, 0) for t in range(d)])
        P.rp.append([morph.Conp(0, 0, t, 0) for t in range(d)])
    P.connect_point(0, 1)
    assert len(P.cnt) == 1 and [(c.li, c.ri) for c in P.cnt[0]] == [((0, t), (1, t)) for t in range(d)]
    P.connect_point(0, 2)  # the left track is connected elsewhere: nothing
    P.connect_point(2, 1)  # the right track is: nothing
    assert len(P.cnt) == 1
    P.connect_point(2, 0)
    assert len(P.cnt) == 2
    P.connect_point(0, 1)  # exactly this pair: removed
    assert len(P.cnt) == 1 and P.cnt[0][0].li == (2, 0)


def test_track_struct_layout():
    assert C.sizeof(capi.TrackSegment) == 32 and C.sizeof(capi.TrackPoint) == 12
    assert morph.TRACK_POINT.itemsize == 12


def test_track_abi_rejects_null_handles(vmlib):
    """NULL handles and a context that is not alive come back as VM_E_INVALID before any device work"""
    h = C.c_void_p()
    assert vmlib.vm_track_create(None, 64, 64, 3, C.byref(h)) == capi.VM_E_INVALID
    assert vmlib.vm_track_create(C.c_void_p(16), 64, 64, 3, C.byref(h)) == capi.VM_E_INVALID
    assert b"context" in vmlib.vm_last_error()
    buf = np.zeros(64 * 64 * 3, np.uint8)
    seg = (capi.TrackSegment * 1)()
    out = np.zeros((1, 3), morph.TRACK_POINT)
    assert vmlib.vm_track_upload_frame(None, 0, 0, buf.ctypes.data, 0) == capi.VM_E_INVALID
    assert vmlib.vm_track_upload_flows(None, 0, 0, None, None, 0) == capi.VM_E_INVALID
    assert vmlib.vm_track_compute_flows(None, None) == capi.VM_E_INVALID
    assert vmlib.vm_track_get_flows(None, 0, 0, None, None) == capi.VM_E_INVALID
    assert vmlib.vm_track_propagate(None, seg, 1, out.ctypes.data) == capi.VM_E_INVALID
    assert vmlib.vm_video_build_flows_track(None, None) == capi.VM_E_INVALID
    assert b"null" in vmlib.vm_last_error().lower()
    vmlib.vm_track_destroy(None)
