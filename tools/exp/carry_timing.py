"""Times of the carry calls (vm_carry.hip) at 1080p on a device-resident frame, and profiles/carry.md from
them.  Three modes:

  carry_timing.py --json PATH          the launches by HIP events (elapsed_ms of the calls, the median of --reps): the
                                       points call at n = 1, 512 and 1 << 20 with nt = 1 and 16, the dense call at
                                       nt = 1, 4 and 16, uniform and under a schedule
  carry_timing.py --loop               the workload of a kernel trace (run it under rocprofv3 --kernel-trace, in a
                                       run of its own): vm_frame_sampling_maps -- which has no timed twin -- and the dense
                                       call at nt = 1, 4, 16, alternating
  carry_timing.py --json PATH --trace KERNEL_TRACE_CSV --out profiles/carry.md
                                       reads both back and writes the table (nothing is run).  The trace is read per
                                       dispatch: the loop's order tells which dense launch had which nt, the first round
                                       of the loop is the warm-up and is left out, and the same statistic -- the median
                                       over the rounds -- stands on both sides of every ratio
The frame holds synth's smooth displacement and no path, the reference application's state."""
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from videomorphing_amd import morph, synth, transition  # noqa: E402

W, H = 1920, 1080
POINT_COUNTS = (1, 512, 1 << 20)
POINT_TIMES = (1, 16)
DENSE_TIMES = (1, 4, 16)


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def times(nt):
    return np.linspace(0.0, 1.0, nt + 2)[1:-1] if nt > 1 else [1.0]


def frame():
    fr = morph.Frame(morph.Context(0), W, H, 0)
    fr.upload_rgb(*synth.make_rgb_pair(W, H))
    fr.upload(v=synth.displacement(W, H).astype(np.float32))
    fr.upload_schedule(transition.wipe(W, H, (1.0, 0.3), lead=0.6, duration=0.4), None)
    return fr


def median_ms(fn, reps):
    fn()                    # warm-up: code objects, allocations
    return float(np.median([fn() for _ in range(reps)]))


def measure(reps):
    fr = frame()
    rng = np.random.RandomState(1)
    out = {"size": [W, H], "reps": reps, "points": [], "dense": []}
    for n in POINT_COUNTS:
        pts = (rng.rand(n, 2) * (W - 1, H - 1)).astype(np.float32)
        for nt in POINT_TIMES:
            out["points"].append({
                "n": n, "nt": nt,
                "uniform_ms": median_ms(lambda: fr.carry_points(pts, 0.5, times(nt), want=("out",), timed=True)[6], reps),
                "scheduled_ms": median_ms(lambda: fr.carry_points_transition(pts, 0.5, times(nt), 1, want=("out",), timed=True)[6], reps)})
    for nt in DENSE_TIMES:
        out["dense"].append({"nt": nt, "uniform_ms": median_ms(lambda: fr.motion_maps_dev(0.5, times(nt)), reps),
                             "scheduled_ms": median_ms(lambda: fr.transition_motion_maps_dev(0.5, times(nt), 1), reps)})
    return out


def loop(reps):
    fr = frame()
    for _ in range(reps + 1):
        fr.sampling_maps(0.5)
        for nt in DENSE_TIMES:
            fr.motion_maps_dev(0.5, times(nt))


def kernel_us(trace_csv):
    """the durations in us, per dispatch and in dispatch order, of the loop's two kernels in a rocprofv3 kernel_trace.csv,
    the warm-up round left out: (maps kernel [rounds], {nt: dense kernel [rounds]})"""
    with open(trace_csv) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Dispatch_Id"]))
    us = lambda name: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if name in r["Kernel_Name"]]
    maps, dense = us("k_warp_win<false, 0, false>"), us("k_motion_win<false, false>")
    assert len(maps) >= 2 and len(dense) == len(DENSE_TIMES) * len(maps), (len(maps), len(dense))
    return maps[1:], {nt: dense[k::len(DENSE_TIMES)][1:] for k, nt in enumerate(DENSE_TIMES)}


def report(j, trace_csv):
    maps, dense = kernel_us(trace_csv)
    maps_us = float(np.median(maps))
    d = {r["nt"]: r for r in j["dense"]}
    L = ["# The carry calls at 1080p (tools/exp/carry_timing.py)", "",
         "A %d x %d frame on the device, synth's smooth displacement, no path; MI355X.  Launch times are HIP events around the"
         % (W, H), "launch (`elapsed_ms` of the calls), the median of %d after a warm-up; a scheduled launch includes its `k_rates`" % j["reps"],
         "pre-pass.  `vm_frame_sampling_maps` has no timed twin: its kernel (`k_warp_win<false, 0, false>`, the code of the parent",
         "commit) and the dense kernel are also read per dispatch from one `rocprofv3 --kernel-trace` run of `--loop`, the median",
         "over its %d rounds after a warm-up round (min - max beside it)." % len(maps), "",
         "## The points call", "", "| n | nt | uniform, us | scheduled, us | what bounds it |", "|---|---|---|---|---|"]
    for r in j["points"]:
        if r["n"] <= 512:
            why = "latency: 21 dependent gathers of one wave per 64 points, and the launch itself; n does not show"
        elif r["nt"] == 1:
            why = "the plain chain's gathers (the texture path and its index arithmetic, DESIGN 3.3): the plain maps kernel's regime"
        else:
            why = "the same chain, plus %d MB of stores" % (r["n"] * r["nt"] * 8 // 1000000)
        L.append("| %d | %d | %.1f | %.1f | %s |" % (r["n"], r["nt"], r["uniform_ms"] * 1e3, r["scheduled_ms"] * 1e3, why))
    L += ["", "## The dense call (motion maps), window form", "",
          "| call | nt | uniform, us | scheduled, us | what bounds it |", "|---|---|---|---|---|",
          "| `vm_frame_sampling_maps` kernel (trace, median) | - | %.1f | - | the chain's taps from the LDS window (DESIGN 3.3), then four stores per pixel (44 MB) |" % maps_us]
    for nt in DENSE_TIMES:
        mb = W * H * (nt * 8 + 5) / 1e6
        why = ("the same chain walked once; %.0f MB of stores" % mb) if nt == 1 else \
              ("the chain once, then %d stores of 16.6 MB each and a dozen flops per to-time: %.0f MB" % (nt, mb))
        L.append("| `vm_frame_motion_maps_dev` | %d | %.1f | %.1f | %s |" % (nt, d[nt]["uniform_ms"] * 1e3, d[nt]["scheduled_ms"] * 1e3, why))
    L += ["", "| kernel (trace) | nt | median, us | min - max, us | of the maps kernel's median |", "|---|---|---|---|---|",
          "| `k_warp_win<false, 0, false>` (`vm_frame_sampling_maps`) | - | %.1f | %.1f - %.1f | 1 |" % (maps_us, min(maps), max(maps))]
    for nt in DENSE_TIMES:
        m = float(np.median(dense[nt]))
        L.append("| `k_motion_win<false, false>` | %d | %.1f | %.1f - %.1f | %.2f |" % (nt, m, min(dense[nt]), max(dense[nt]), m / maps_us))
    L += ["", "Median beside median over the same %d rounds: the dense kernel at nt = 1 takes %.2f of the maps' kernel time." %
          (len(maps), float(np.median(dense[1])) / maps_us),
          "By events a further to-time costs %.1f us between nt = 1 and 4 and %.1f us between nt = 4 and 16: a to-time's 16.6 MB of"
          % ((d[4]["uniform_ms"] - d[1]["uniform_ms"]) * 1e3 / 3, (d[16]["uniform_ms"] - d[4]["uniform_ms"]) * 1e3 / 12),
          "stores leave while other workgroups walk their chains, so few of them cost time of their own; at nt = 16 the %.0f MB in %.1f us"
          % (W * H * 133 / 1e6, d[16]["uniform_ms"] * 1e3),
          "are %.1f TB/s and the stores begin to show.  A scheduled chain reads a third window (the rates) and its launch includes"
          % (W * H * 133 / 1e6 / (d[16]["uniform_ms"] * 1e3)),
          "`k_rates`; its tail ramps four schedule texels per to-time (a division each).", ""]
    return "\n".join(L)


def main():
    reps = int(arg("--reps", 5))
    if "--loop" in sys.argv:
        return loop(reps)
    path = arg("--json")
    if "--trace" in sys.argv:
        with open(path) as f:
            text = report(json.load(f), arg("--trace"))
        with open(arg("--out"), "w") as f:
            f.write(text)
        return print(text)
    out = measure(reps)
    print(json.dumps(out))
    if path:
        with open(path, "w") as f:
            json.dump(out, f)


if __name__ == "__main__":
    main()
