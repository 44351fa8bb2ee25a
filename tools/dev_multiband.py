"""Times the multiband render calls at 1080p beside the calls they extend, in one GPU process:

  vm_render_halfway_dev            beside  vm_frame_render_multiband_dev
  vm_render_layers_dev (1, 4 ch)   beside  vm_frame_render_multiband_layers_dev

on one frame with ex = 192, a solver-shaped smooth field (with and without a path) and L = 5 bands, device events around each
call.  Two rounds of warm-up, then `--reps` rounds in which the calls alternate; medians, and the multiband call's ratio to
its plain counterpart.

  python tools/dev_multiband.py [--reps N] [--size WxH] [--out PATH]     the events table (default: profiles/multiband.md)
  python tools/dev_multiband.py --loop N                                 the workload of a kernel trace: N rounds of the
                                                                         three multiband calls, nothing timed (run it under
                                                                         rocprofv3 --kernel-trace, in a run of its own)
  python tools/dev_multiband.py --trace KERNEL_TRACE.csv [--out PATH]    appends the split per kernel to the note: medians per
                                                                         kernel and level, and for the level-0 reduce and
                                                                         collapse the algorithmic bytes over the time as a
                                                                         fraction of 8 TB/s (needs no GPU)
Development tool: the numbers gate nothing.
"""
import argparse
import csv
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

f32 = np.float32
FA, EX, LEVELS = 0.37, 192, 5
PEAK = 8e12         # bytes per second


def frame_of(w, h):
    from videomorphing_amd import capi, morph, synth
    ctx = morph.Context(0, capi.MATH_FAST)
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    rng = np.random.RandomState(3)
    d = synth.displacement(w, h)
    v = (d + 0.05 * rng.randn(h, w, 2)).astype(f32)                 # a solved field: smooth, rounding-rough
    u = (0.25 * d[..., ::-1]).astype(f32)
    layers = {c: (rng.rand(h, w, c).astype(f32), rng.rand(h, w, c).astype(f32)) for c in (1, 4)}
    fr = morph.Frame(ctx, w, h, EX)
    e0, e1 = morph.make_extended(rgb0, EX), morph.make_extended(rgb1, EX)
    return ctx, fr, (e0, e1, v, u), layers


def events(a):
    from videomorphing_amd.multiband import Bands
    w, h = (int(x) for x in a.size.split("x"))
    ctx, fr, (e0, e1, v, u), layers = frame_of(w, h)
    name, cus, _ = ctx.device_info()
    bands = Bands.sharpen(LEVELS, 4)
    rows = []
    for with_path in (False, True):
        fr.upload(e0, e1, v, u if with_path else None)
        ts = {}
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {("RGB8", "plain"): fr.render_halfway_dev(FA, FA, 1), ("RGB8", "bands"): fr.render_multiband_dev(bands, FA, FA)}
            for ch in (1, 4):
                fr.upload_layers(*layers[ch])
                fr.render_layers_dev(FA, FA, 1)                     # (the first launch after an upload is not the timed one)
                got[("%d ch" % ch, "plain")] = fr.render_layers_dev(FA, FA, 1)
                got[("%d ch" % ch, "bands")] = fr.render_multiband_layers_dev(bands, FA, FA)
            if rep >= 2:
                for k, t in got.items():
                    ts.setdefault(k, []).append(t)
        rows.append((with_path, {k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ts.items()}))
    lines = [
        "# The multiband render calls at %dx%d beside the calls they extend" % (w, h),
        "",
        "Measured by `tools/dev_multiband.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls alternating" % (name.strip(), cus, a.reps),
        "within a round.  ex = %d, a smooth solver-shaped field, L = %d bands (`Bands.sharpen(%d, 4)`), color_fa = geo_fa = %.2f." % (EX, LEVELS, LEVELS, FA),
        "Device events around each call, ms: median (min .. max); `x`: the multiband call over the plain one.  The numbers gate nothing.",
        "",
        "| tail | path | plain call | multiband call | x |",
        "|---|---|---|---|---|",
    ]
    for tail in ("RGB8", "1 ch", "4 ch"):
        for with_path, ts in rows:
            p, b = ts[(tail, "plain")], ts[(tail, "bands")]
            lines.append("| %s | %s | %.4f (%.4f .. %.4f) | %.4f (%.4f .. %.4f) | %.2f |" % ((tail, "yes" if with_path else "no") + p + b + (b[0] / p[0],)))
    lines.append("")
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def loop(a):
    from videomorphing_amd.multiband import Bands
    w, h = (int(x) for x in a.size.split("x"))
    ctx, fr, (e0, e1, v, u), layers = frame_of(w, h)
    bands = Bands.sharpen(LEVELS, 4)
    fr.upload(e0, e1, v, u)
    for _ in range(a.loop):
        fr.render_multiband_dev(bands, FA, FA)
        for ch in (1, 4):
            fr.upload_layers(*layers[ch])
            fr.render_multiband_layers_dev(bands, FA, FA)
    print("looped %d rounds" % a.loop)


def trace(a):
    """the split per kernel from one kernel trace of --loop: a call's kernels are told apart by name (the warp pass and the
    collapse carry the channel count), a reduce's and a collapse's level by its grid"""
    w, h = (int(x) for x in a.size.split("x"))
    sizes = [(w, h)]
    for _ in range(LEVELS):
        sizes.append(((sizes[-1][0] + 1) // 2, (sizes[-1][1] + 1) // 2))
    with open(a.trace) as f:
        rows = [r for r in csv.DictReader(f) if "k_mb_" in r["Kernel_Name"]]
    groups = {}
    for r in rows:
        n = re.search(r"k_mb_\w+(<[^>]*>)?", r["Kernel_Name"]).group(0)
        gx, gy, gz = (int(r["Grid_Size_" + c]) // int(r["Workgroup_Size_" + c]) for c in "XYZ")
        level = ""
        if "reduce" in n or "collapse" in n:
            for l, (lw, lh) in enumerate(sizes):
                if ((lw + 31) // 32, (lh + 7) // 8) == (gx, gy):
                    level = "%d" % (l - 1 if "reduce" in n else l)      # a reduce's grid is its output's: level l into l + 1
        if "reduce" in n:
            n += " x %d planes" % gz
        groups.setdefault((n, level), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    lines = ["", "## The split per kernel", "",
             "One `rocprofv3 --kernel-trace` run of `tools/dev_multiband.py --loop` (a run of its own, with a path): the RGB8 call and the",
             "layer calls of 1 and 4 channels, us per dispatch, medians.  For the level-0 reduce and collapse the algorithmic bytes --",
             "the reduce reads 8 C + 4 bytes per pixel and writes a quarter of it; the collapse reads 8 C + 4 and a quarter of 12 C from",
             "level 1 and writes 3 (RGB8) or 4 C -- over the time, as a fraction of 8 TB/s.", "",
             "| kernel | level | dispatches | median us | min | bytes / time | of 8 TB/s |", "|---|---|---|---|---|---|---|"]
    px = w * h
    for (n, level), ts in sorted(groups.items()):
        med, extra = float(np.median(ts)), " | |"
        if level == "0":
            c = None
            if "reduce" in n:
                c = (int(n.split(" x ")[1].split()[0]) - 1) // 2
                nbytes = px * (8 * c + 4) * 1.25
            elif "collapse" in n:
                c, out = (int(x) for x in n.split("<")[1].rstrip(">").split(","))
                nbytes = px * ((8 * c + 4) + 12 * c / 4 + (3 if out == 2 else 4 * c))
            if c:
                rate = nbytes / (med * 1e-6)
                extra = " %.2f TB/s | %.0f %% |" % (rate / 1e12, 100 * rate / PEAK)
        lines.append("| `%s` | %s | %d | %.1f | %.1f |%s" % (n, level, len(ts), med, min(ts), extra))
    lines.append("")
    with open(a.out, "a") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multiband.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--loop", type=int, default=0)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        trace(a)
    elif a.loop:
        loop(a)
    else:
        events(a)


if __name__ == "__main__":
    main()
