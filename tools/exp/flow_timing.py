"""Times of the dense optical flow (vm_flow.hip) at 1080p: one flow alone, the 60 flows of a
16-frame video pair in one call (4 x 15 frame pairs), and the 30 forward flows of the sync stage
computed from frames already on the device.  Each C-ABI call drains its stream before it returns,
so the host clock around a call is its full time (uploads and downloads included where the call
makes them); per-kernel device times come from a rocprofv3 --kernel-trace --stats run of this
script (profiles/flow_1080p_kernels.md).  Prints one JSON line; --quick: one repetition each;
--out PATH: also write the JSON there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from videomorphing_amd import morph, synth  # noqa: E402


def timed(fn, reps):
    fn()  # warm-up: code objects, allocations
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    reps = 1 if "--quick" in sys.argv else 3
    w, h, d = 1920, 1080, 16
    ctx = morph.Context(0)
    fr = [synth.make_video_pair(w, h, t, (6.0, -3.5), (1.5, -0.25)) for t in range(d)]
    v0 = np.stack([f[0] for f in fr])
    v1 = np.stack([f[1] for f in fr])
    out = {"size": [w, h]}
    out["one_flow_ms"] = timed(lambda: morph.optical_flow(ctx, v0[0], v0[1]), reps)
    out["video_pair_60_flows_ms"] = timed(lambda: morph.video_optical_flows(ctx, v0, v1), reps)
    out["video_pair_ms_per_flow"] = out["video_pair_60_flows_ms"] / 60
    grey = lambda v: np.repeat(np.clip(np.rint(v), 0, 255).astype(np.uint8)[..., None], 3, -1)
    sp = morph.SyncPyramid(ctx)
    z = np.zeros((d, h, w, 2), np.float32)
    sp.build(grey(v0), grey(v1), z, z, 16)
    out["sync_30_flows_device_frames_ms"] = timed(sp.compute_flows, reps)
    out["sync_ms_per_flow"] = out["sync_30_flows_device_frames_ms"] / 30
    print(json.dumps(out))
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
