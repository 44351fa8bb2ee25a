"""The stage-2 point tracker's spec in numpy / plain Python doubles: MdiEditor's
AddPoint / MovePoint (UI/MdiEditor.cpp:1230-1393), Histo (:1516-1582) and NextStage's points section
(:1714-1791), written two ways:

- literally: `add_point` / `move_point` edit a track (a list of [x, y, z, w, weight], one per frame)
  in the reference's order;
- as segments: `key_segments` turns the keys a sequence of edits leaves (with the time each was last
  edited) into chain and blend segments, `run_segment` computes one -- what vm_track.hip does.

A video is (d, h, w, 3) uint8, a flow family (d, h, w, 2) float32; f[t] maps t -> t + 1, b[t] t -> t - 1.
"""
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
# calcHist's uniform 8-bit lookup for 10 bins over [0, 255): floor(v * (10.0 / 255.0)) in double, 255 uncounted
BIN = [int(math.floor(v * (10.0 / 255.0))) for v in range(255)]


def step(x, y, F):
    """pt.p.x += F.x + 0.5 on an int (:1241-1249): int += float + double, truncation toward zero"""
    return int(float(x) + (float(np.float32(F[0])) + 0.5)), int(float(y) + (float(np.float32(F[1])) + 0.5))


def flow_step(x, y, flow):
    """one step along a (h, w, 2) flow, read at the clamped point; the point itself is not clamped"""
    h, w = flow.shape[:2]
    return step(x, y, flow[min(max(y, 0), h - 1), min(max(x, 0), w - 1)])


def patch_hist(frame, x, y):
    """calcHist of the patch cv::Range(cl(y-3), cl(y+3)) x cv::Range(cl(x-3), cl(x+3)): 1000 counts"""
    h, w = frame.shape[:2]
    cl = lambda v, n: min(max(v, 0), n - 1)
    hist = np.zeros(1000, np.int64)
    for yy in range(cl(y - 3, h), cl(y + 3, h)):
        for xx in range(cl(x - 3, w), cl(x + 3, w)):
            r, g, b = (int(c) for c in frame[yy, xx, :3])
            if r < 255 and g < 255 and b < 255:
                hist[BIN[r] * 100 + BIN[g] * 10 + BIN[b]] += 1
    return hist


def correl(h1, h2):
    """compareHist(h1, h2, HISTCMP_CORREL), fabs, as float32: exact integer sums, then doubles"""
    s1, s2 = int(h1.sum()), int(h2.sum())
    s11, s22, s12 = int((h1 * h1).sum()), int((h2 * h2).sum()), int((h1 * h2).sum())
    scale = 1.0 / 1000
    num = s12 - (s1 * s2) * scale
    den2 = (s11 - (s1 * s1) * scale) * (s22 - (s2 * s2) * scale)
    r = num / math.sqrt(den2) if abs(den2) > DBL_EPSILON else 1.0
    return np.float32(abs(r))


def histo(video, p, q):
    """Histo(p, q): the patch of p in frame p.z against the patch of q in frame q.z, one video"""
    return correl(patch_hist(video[p[2]], p[0], p[1]), patch_hist(video[q[2]], q[0], q[1]))


# ---- the literal edits ----------------------------------------------------------------------------

def add_point(video, f, b, key):
    """AddPoint (:1230-1276): a new track from key (x, y, z); returns its d entries [x, y, z, w, weight]"""
    d = len(video)
    x0, y0, z0 = key
    pts = [[x0, y0, z0, 1, np.float32(1.0)]]
    x, y = x0, y0
    for t in range(z0, 0, -1):
        x, y = flow_step(x, y, b[t])
        pts.insert(0, [x, y, t - 1, 0, histo(video, (x, y, t - 1), key)])
    x, y = x0, y0
    for t in range(z0, d - 1):
        x, y = flow_step(x, y, f[t])
        pts.append([x, y, t + 1, 0, histo(video, (x, y, t + 1), key)])
    return pts


def move_point(video, f, b, pts, mid):
    """MovePoint (:1279-1393) after the caller has put the moved key at pts[mid]"""
    f32 = np.float32
    km = tuple(pts[mid][:3])
    beg = -1
    for j in range(mid - 1, -1, -1):
        if pts[j][3]:
            beg = j
            break
    x, y = km[0], km[1]
    for t in range(mid, beg + 1, -1):
        x, y = flow_step(x, y, b[t])
        pts[t - 1] = [x, y, t - 1, 0, histo(video, (x, y, t - 1), km)]
    if beg >= 0:
        kb = tuple(pts[beg][:3])
        x, y = kb[0], kb[1]
        for t in range(beg, mid - 1):
            fa = f32(f32((t + 1) - beg) / f32(mid - beg))
            x, y = flow_step(x, y, f[t])
            q = pts[t + 1]
            q[0] = int(f32(f32(q[0]) * fa) + f32(f32(x) * f32(f32(1) - fa)))
            q[1] = int(f32(f32(q[1]) * fa) + f32(f32(y) * f32(f32(1) - fa)))
            p = (q[0], q[1], q[2])
            q[4] = f32(f32(histo(video, p, km) * fa) + f32(histo(video, p, kb) * f32(f32(1) - fa)))
    end = len(pts)
    for j in range(mid + 1, len(pts)):
        if pts[j][3]:
            end = j
            break
    x, y = km[0], km[1]
    for t in range(mid, end - 1):
        x, y = flow_step(x, y, f[t])
        pts[t + 1] = [x, y, t + 1, 0, histo(video, (x, y, t + 1), km)]
    if end < len(pts):
        ke = tuple(pts[end][:3])
        x, y = ke[0], ke[1]
        for t in range(end, mid + 1, -1):
            fa = f32(f32(end - (t - 1)) / f32(end - mid))
            x, y = flow_step(x, y, b[t])
            q = pts[t - 1]
            q[0] = int(f32(f32(q[0]) * fa) + f32(f32(x) * f32(f32(1) - fa)))
            q[1] = int(f32(f32(q[1]) * fa) + f32(f32(y) * f32(f32(1) - fa)))
            p = (q[0], q[1], q[2])
            q[4] = f32(f32(histo(video, p, km) * fa) + f32(histo(video, p, ke) * f32(f32(1) - fa)))
    return pts


def edit_sequence(video, f, b, edits):
    """edits: [(x, y, z), ...] in order; the first is AddPoint, each later one replaces frame z, then MovePoint"""
    pts = add_point(video, f, b, edits[0])
    for x, y, z in edits[1:]:
        pts[z] = [x, y, z, 1, np.float32(1.0)]
        move_point(video, f, b, pts, z)
    return pts


# ---- the segment form -----------------------------------------------------------------------------

def chain(video, f, b, key, direction):
    """{frame: (x, y, weight)} from key (x, y, z) in direction +-1 up to the last / first frame"""
    d = len(video)
    out = {}
    x, y = key[0], key[1]
    s = key[2] + direction
    while 0 <= s < d:
        x, y = flow_step(x, y, (f if direction > 0 else b)[s - direction])
        out[s] = (x, y, histo(video, (x, y, s), key))
        s += direction
    return out


def blend(video, f, b, m, o):
    """{frame: (x, y, weight)} strictly between the moved key m and the neighbouring key o"""
    f32 = np.float32
    dr = 1 if o[2] > m[2] else -1
    co = {}
    x, y = o[0], o[1]
    for s in range(o[2] - dr, m[2], -dr):
        x, y = flow_step(x, y, (f if dr < 0 else b)[s + dr])
        co[s] = (x, y)
    out = {}
    x, y = m[0], m[1]
    for s in range(m[2] + dr, o[2], dr):
        x, y = flow_step(x, y, (f if dr > 0 else b)[s - dr])
        fa = f32(f32(abs(o[2] - s)) / f32(abs(o[2] - m[2])))
        px = int(f32(f32(x) * fa) + f32(f32(co[s][0]) * f32(f32(1) - fa)))
        py = int(f32(f32(y) * fa) + f32(f32(co[s][1]) * f32(f32(1) - fa)))
        p = (px, py, s)
        out[s] = (px, py, f32(f32(histo(video, p, m) * fa) + f32(histo(video, p, o) * f32(f32(1) - fa))))
    return out


def final_keys(edits):
    """the keys a sequence of edits leaves: {z: ((x, y, z), time of its last edit)}"""
    keys = {}
    for i, (x, y, z) in enumerate(edits):
        keys[z] = ((x, y, z), i)
    return keys


def key_segments(keys):
    """keys {z: (key, time)} -> [("chain", key, dir) | ("blend", m, o)]: chains before the first and
    after the last key, a blend between adjacent keys whose m is the one edited later"""
    zs = sorted(keys)
    segs = [("chain", keys[zs[0]][0], -1), ("chain", keys[zs[-1]][0], 1)]
    for a, c in zip(zs, zs[1:]):
        (ka, ta), (kc, tc) = keys[a], keys[c]
        segs.append(("blend", ka, kc) if ta > tc else ("blend", kc, ka))
    return segs


def run_segment(video, f, b, seg):
    return chain(video, f, b, seg[1], seg[2]) if seg[0] == "chain" else blend(video, f, b, seg[1], seg[2])


def segment_track(video, f, b, edits):
    """the track edit_sequence leaves, from the segment form"""
    keys = final_keys(edits)
    pts = [None] * len(video)
    for z, (k, _) in keys.items():
        pts[z] = [k[0], k[1], z, 1, np.float32(1.0)]
    for seg in key_segments(keys):
        for s, (x, y, wt) in run_segment(video, f, b, seg).items():
            pts[s] = [x, y, s, 0, wt]
    return pts


# ---- NextStage ------------------------------------------------------------------------------------

def next_stage_edits(lp, rp, cnt):
    """NextStage's points section (:1714-1791) as edit lists: for stage-1 list i, connection j becomes a key
    at z = (lz + rz) / 2 (integer division, then + 0.5 truncated) on the left track i and the right track i.
    lp / rp: tracks of (x, y, z) points, cnt: lists of ((li_track, li_index), (ri_track, ri_index)).
    Returns ([left edits per list], [right edits per list])."""
    le, re_ = [], []
    for row in cnt:
        a, c = [], []
        for li, ri in row:
            l, r = lp[li[0]][li[1]], rp[ri[0]][ri[1]]
            z = int((l[2] + r[2]) // 2 + 0.5)
            a.append((l[0], l[1], z))
            c.append((r[0], r[1], z))
        le.append(a)
        re_.append(c)
    return le, re_


def next_stage(videos, flows, lp, rp, cnt):
    """the literal NextStage: tracks per side (lists of [x, y, z, w, weight]) and the per-frame connects"""
    d = len(videos[0])
    le, re_ = next_stage_edits(lp, rp, cnt)
    tracks = [[edit_sequence(videos[k], flows[k][0], flows[k][1], e) for e in edits] for k, edits in enumerate((le, re_))]
    cnt2 = [[((i, t), (i, t)) for t in range(d)] for i in range(len(le))]
    return tracks[0], tracks[1], cnt2
