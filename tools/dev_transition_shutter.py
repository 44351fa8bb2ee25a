"""Times the shutter calls under a transition schedule at 1080p beside what they replace and what they extend, in one GPU
process:

  vm_render_transition_shutter_dev(N)                 beside N x vm_render_transition_dev at the shutter's sample times
                                                      (a rate pre-pass per sample: the route the fused call does not take)
                                                      and vm_render_shutter_dev(N) (no schedule: what the rates cost)
  vm_render_transition_shutter_layers_dev(N), 1, 4 ch beside N x vm_render_transition_layers_dev and
                                                      vm_render_shutter_layers_dev(N)
  vm_render_transition_shutter (with its download)    beside the host route: N x vm_render_transition and a float mean in
                                                      numpy

for N = 4, 8, 16 and shutters 0.02 wide (consecutive windows mostly coincide) and 0.5 wide (they do not), centred on
t = 0.5, the colour at 0.5, linear ease, with and without a path, device events around each call.  The field is that of
tools/dev_layer_warp.py (profiles/layer_warp.md), the schedule videomorphing_amd.transition.wipe's default on both
planes.  A warm-up of every call, then `--reps` rounds in which the calls alternate; medians, and for the N transition
calls the minimum and maximum of the rounds' sums as well (their run-to-run spread is the yardstick).  The host route is
wall-clock, `--host-reps` times.  A 1-channel layer call with N = 4 is compared bit for bit with the float32 sum of the
transition kernel's results at the sample times of tests/transit_shutter_ref.py, divided once -- with a uniform colour
schedule, under which the colour rate does not depend on the time.  Writes a markdown note (default:
profiles/transition_shutter.md).  Development tool: the numbers gate nothing.

  python tools/dev_transition_shutter.py [--out PATH] [--reps N] [--host-reps N] [--size WxH] [--label TEXT] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transit_shutter_ref as TS  # noqa: E402
from videomorphing_amd import capi, morph, synth, transition  # noqa: E402

f32 = np.float32
NS = (4, 8, 16)
WIDTHS = (0.02, 0.5)
T_COLOR = 0.5
EASE = capi.EASE_LINEAR
KINDS = ("rgb", "l1", "l4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transition_shutter.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--label", default="the product build")
    ap.add_argument("--append", action="store_true")
    a = ap.parse_args()
    w, h = (int(x) for x in a.size.split("x"))
    ex = 24
    ctx = morph.Context(0, capi.MATH_FAST)
    name, cus, _ = ctx.device_info()
    rgb0, rgb1 = synth.make_rgb_pair(w, h)
    rng = np.random.RandomState(3)
    d = synth.displacement(w, h)
    v = (d + 0.05 * rng.randn(h, w, 2)).astype(f32)                 # a solved field: smooth, rounding-rough
    u = (0.25 * d[..., ::-1]).astype(f32)
    layers = {c: ((rng.rand(h, w, c).astype(f32)), (rng.rand(h, w, c).astype(f32))) for c in (1, 4)}
    wipe = transition.wipe(w, h)
    fr = morph.Frame(ctx, w, h, ex)
    rows = []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        fr.upload_schedule(wipe, wipe)
        for width in WIDTHS:
            o, c = 0.5 - width / 2, 0.5 + width / 2
            for n in NS:
                times = [float(t) for t in TS.sample_times(o, c, n)]
                ts = {k + s: [] for k in KINDS for s in ("", "_n", "_u")}
                for rep in range(a.reps + 2):                       # two rounds of warm-up
                    got = {"rgb": fr.render_transition_shutter_dev(o, c, n, T_COLOR, EASE, 1),
                           "rgb_n": sum(fr.render_transition_dev(t, EASE, 1) for t in times),
                           "rgb_u": fr.render_shutter_dev(T_COLOR, o, c, n, 1)}
                    for ch in (1, 4):
                        fr.upload_layers(*layers[ch])
                        fr.render_layers_dev(T_COLOR, 0.5, 1)       # (the first launch after an upload is not the timed one)
                        got["l%d" % ch] = fr.render_transition_shutter_layers_dev(o, c, n, T_COLOR, EASE, 1)
                        got["l%d_n" % ch] = sum(fr.render_transition_layers_dev(t, EASE, 1) for t in times)
                        got["l%d_u" % ch] = fr.render_shutter_layers_dev(T_COLOR, o, c, n, 1)
                    if rep >= 2:
                        for k in ts:
                            ts[k].append(got[k])
                host, fused = [], []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    acc = np.zeros((h, w, 3), f32)
                    for t in times:
                        acc += fr.render_transition(t, EASE, 1)
                    mean = acc / f32(n)
                    host.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    img = fr.render_transition_shutter(o, c, n, T_COLOR, EASE, 1)
                    fused.append(1e3 * (time.perf_counter() - t0))
                # (the host route rounds every sample to 8 bits first, and its colour rate moves with the sample time)
                off = float(np.abs(mean - img).max())
                rows.append((with_path, width, n, {k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ts.items()},
                             float(np.median(host)), float(np.median(fused)), off))
        # what was timed is what is specified: under a uniform colour schedule and color_from 0 the fused call is the
        # float32 sum, in sample order, of the transition kernel's own results (which tests/test_gpu_transition.py holds to
        # the statement), divided once
        fr.upload_schedule(wipe, None)
        fr.upload_layers(*layers[1])
        acc = np.zeros((h, w, 1), f32)
        for t in TS.sample_times(0.25, 0.75, 4):
            acc = acc + fr.render_transition_layers(float(t), EASE, 0)
        got = fr.render_transition_shutter_layers(0.25, 0.75, 4, T_COLOR, EASE, 0)
        assert np.array_equal(got.view(np.uint32), (acc / f32(4)).view(np.uint32))
    lines = [
        "%s The shutter calls under a schedule at %dx%d beside N transition renders and the uniform shutter: %s" % ("##" if a.append else "#", w, h, a.label),
        "",
        "Measured by `tools/dev_transition_shutter.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls" % (name.strip(), cus, a.reps),
        "alternating within a round.  Field and path: those of `profiles/layer_warp.md`; schedule: `transition.wipe`'s default on",
        "both planes.  Shutters centred on t = 0.5, t_color %.1f, linear ease, color_from 1.  Device events around each call, ms:" % T_COLOR,
        "the fused call's median (`fused`); for the N transition calls at the same sample times the median of their sum",
        "(minimum .. maximum over the rounds: the yardstick) and the fused call's ratio to it (`/ N x`); the uniform shutter call",
        "at the same N and the fused call's ratio to it (`/ uniform`).  Host route: wall-clock ms, N x `vm_render_transition` with",
        "a float mean in numpy beside `vm_render_transition_shutter` with its download, median of %d; `off` is the largest" % a.host_reps,
        "difference of the two pictures in grey levels (the host route rounds every sample to 8 bits and lets the colour rate move",
        "with the sample time).  The numbers gate nothing.",
        "",
        "| path | width | N | " + " | ".join("fused %s | N x transition | / N x | uniform shutter | / uniform" % k for k in ("RGB8", "1 ch", "4 ch"))
        + " | host route | fused + download | off |",
        "|---|---|---|" + "---|" * (5 * len(KINDS)) + "---|---|---|",
    ]
    for with_path, width, n, ts, host, fused, off in rows:
        cells = []
        for k in KINDS:
            f, nx, un = ts[k], ts[k + "_n"], ts[k + "_u"]
            cells += ["%.4f" % f[0], "%.4f (%.4f .. %.4f)" % nx, "%.2f" % (f[0] / nx[0]), "%.4f" % un[0], "%.2f" % (f[0] / un[0])]
        lines.append("| %s | %.2f | %d | %s | %.1f | %.1f | %.2f |" % ("yes" if with_path else "no", width, n, " | ".join(cells), host, fused, off))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
