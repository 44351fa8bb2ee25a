"""Times of the stage-2 point tracker (vm_track.hip) on a 1080p x 60-frame video pair: the flows of
both videos on the device (vm_track_compute_flows, 2 x 2 x 59 flows) and ONE vm_track_propagate call
of 64 tracks x 3 keys on both sides (per track and side two chains and two blends: 512 segments).
Each C-ABI call drains its stream before it returns, so the host clock around a call is its full
time (the propagate call includes its segment upload and result download).  Prints one JSON line;
--quick: one repetition each; --out PATH: also write the JSON there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from videomorphing_amd import capi, morph  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: code objects, allocations
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def video(w, h, d, shift, seed):
    """a smooth random texture translating by whole pixels per frame, RGB8"""
    rng = np.random.default_rng(seed)
    base = rng.random((h // 8 + 2, w // 8 + 2, 3))
    base = np.repeat(np.repeat(base, 8, 0), 8, 1)
    tex = (base[:h, :w] * 200 + 20).astype(np.uint8)
    return np.stack([np.roll(tex, (t * shift[1], t * shift[0]), (0, 1)) for t in range(d)])


def main():
    reps = 1 if "--quick" in sys.argv else 3
    w, h, d = 1920, 1080, 60
    ctx = morph.Context(0)
    v0, v1 = video(w, h, d, (2, -1), 1), video(w, h, d, (-1, 1), 2)
    tr = morph.PointTracker(ctx, v0, v1)  # computes the flows once (the warm-up)
    out = {"size": [w, h], "depth": d}
    out["compute_flows_ms"] = timed(lambda: capi.check(tr._L.vm_track_compute_flows(tr._h, None)), reps)
    rng = np.random.default_rng(3)
    segs = []
    for side in range(2):
        for _ in range(64):
            zs = sorted(rng.choice(d, 3, replace=False).tolist())
            keys = [(int(rng.integers(0, w)), int(rng.integers(0, h)), int(z)) for z in zs]
            segs += [("chain", keys[0], -1), ("chain", keys[2], 1), ("blend", keys[1], keys[0]), ("blend", keys[1], keys[2])]
            segs[-4:] = [morph._segment_tuple(side, s) for s in segs[-4:]]
    out["segments"] = len(segs)
    out["propagate_ms"] = timed(lambda: tr.propagate(segs), reps)
    out["propagate_one_segment_ms"] = timed(lambda: tr.propagate(segs[:1]), reps)
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
