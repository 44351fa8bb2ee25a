"""Times the shutter calls at 1080p beside what they replace, in one GPU process:

  vm_render_shutter_dev(N)                    beside N x vm_render_halfway_dev at the shutter's sample times
  vm_render_shutter_layers_dev(N), 1, 3, 4 ch beside N x vm_render_layers_dev
  vm_render_shutter (with its download)       beside the host route: N x vm_render_halfway and a float mean in numpy

for N = 1, 4, 8, 16 and shutters 0.02 wide (consecutive windows mostly coincide) and 0.5 wide (they do not), centred on
t = 0.5, with and without a path, device events around each call.  The field is that of tools/dev_layer_warp.py
(profiles/layer_warp.md).  A warm-up of every call, then `--reps` rounds in which the calls alternate; medians, and for the
N uniform calls the minimum and maximum of the rounds' sums as well (their run-to-run spread is the yardstick).  The host
route is wall-clock, `--host-reps` times.  A 1-channel layer call with N = 4 is compared bit for bit with the float32 sum of
the uniform kernel's results at the sample times of tests/shutter_ref.py, divided once.  Writes a markdown note (default:
profiles/shutter.md); `--label` names the build in it (a variant library is loaded with VM_LIB_PATH) and `--append` adds
the run to the note as a further section instead of replacing it.  Development tool: the numbers gate nothing.

  python tools/dev_shutter.py [--out PATH] [--reps N] [--host-reps N] [--size WxH] [--label TEXT] [--append]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import shutter_ref as S  # noqa: E402
from videomorphing_amd import capi, morph, synth  # noqa: E402

f32 = np.float32
NS = (1, 4, 8, 16)
WIDTHS = (0.02, 0.5)
COLOR_FA = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shutter.md"))
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
    layers = {c: ((rng.rand(h, w, c).astype(f32)), (rng.rand(h, w, c).astype(f32))) for c in (1, 3, 4)}
    fr = morph.Frame(ctx, w, h, ex)
    rows = []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        for width in WIDTHS:
            o, c = 0.5 - width / 2, 0.5 + width / 2
            for n in NS:
                times = [float(t) for t in S.sample_times(o, c, n)]
                ts = {k: [] for k in ("rgb", "rgb_n", "l1", "l1_n", "l3", "l3_n", "l4", "l4_n")}
                for rep in range(a.reps + 2):                       # two rounds of warm-up
                    got = {"rgb": fr.render_shutter_dev(COLOR_FA, o, c, n, 1),
                           "rgb_n": sum(fr.render_halfway_dev(COLOR_FA, t, 1) for t in times)}
                    for ch in (1, 3, 4):
                        fr.upload_layers(*layers[ch])
                        fr.render_layers_dev(COLOR_FA, 0.5, 1)      # (the first launch after an upload is not the timed one)
                        got["l%d" % ch] = fr.render_shutter_layers_dev(COLOR_FA, o, c, n, 1)
                        got["l%d_n" % ch] = sum(fr.render_layers_dev(COLOR_FA, t, 1) for t in times)
                    if rep >= 2:
                        for k in ts:
                            ts[k].append(got[k])
                host, fused = [], []
                for _ in range(a.host_reps):
                    t0 = time.perf_counter()
                    acc = np.zeros((h, w, 3), f32)
                    for t in times:
                        acc += fr.render_halfway(COLOR_FA, t, 1)
                    mean = acc / f32(n)
                    host.append(1e3 * (time.perf_counter() - t0))
                    t0 = time.perf_counter()
                    img = fr.render_shutter(COLOR_FA, o, c, n, 1)
                    fused.append(1e3 * (time.perf_counter() - t0))
                off = float(np.abs(mean - img).max())               # (the host route rounds every sample to 8 bits first)
                rows.append((with_path, width, n, {k: (float(np.median(x)), float(np.min(x)), float(np.max(x))) for k, x in ts.items()},
                             float(np.median(host)), float(np.median(fused)), off))
        # what was timed is what is specified: the fused call is the float32 sum, in sample order, of the uniform kernel's
        # own results (which tests/test_gpu_layers.py holds to the statement), divided once
        fr.upload_layers(*layers[1])
        acc = np.zeros((h, w, 1), f32)
        for t in S.sample_times(0.25, 0.75, 4):
            acc = acc + fr.render_layers(COLOR_FA, float(t), 1)
        got = fr.render_shutter_layers(COLOR_FA, 0.25, 0.75, 4, 1)
        assert np.array_equal(got.view(np.uint32), (acc / f32(4)).view(np.uint32))
    lines = [
        "%s The shutter calls at %dx%d beside N uniform renders: %s" % ("##" if a.append else "#", w, h, a.label),
        "",
        "Measured by `tools/dev_shutter.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls alternating" % (name.strip(), cus, a.reps),
        "within a round.  Field and path: those of `profiles/layer_warp.md`.  Shutters centred on t = 0.5, color_fa %.1f," % COLOR_FA,
        "color_from 1.  Device events around each call, ms: the fused call's median, and for the N uniform calls at the same",
        "sample times the median of their sum (minimum .. maximum over the rounds: the yardstick).  Host route: wall-clock ms,",
        "N x `vm_render_halfway` with a float mean in numpy beside `vm_render_shutter` with its download, median of %d;" % a.host_reps,
        "`off` is the largest difference of the two pictures in grey levels (the host route rounds every sample to 8 bits).",
        "The numbers gate nothing.",
        "",
        "| path | width | N | shutter RGB8 | N x halfway | ratio | shutter 1 ch | N x layers 1 ch | ratio | shutter 3 ch | N x layers 3 ch | ratio | shutter 4 ch | N x layers 4 ch | ratio | host route | fused + download | off |",
        "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|",
    ]
    for with_path, width, n, ts, host, fused, off in rows:
        cells = []
        for k in ("rgb", "l1", "l3", "l4"):
            f, u3 = ts[k], ts[k + "_n"]
            cells += ["%.4f" % f[0], "%.4f (%.4f .. %.4f)" % u3, "%.2f" % (f[0] / u3[0])]
        lines.append("| %s | %.2f | %d | %s | %.1f | %.1f | %.2f |" % ("yes" if with_path else "no", width, n, " | ".join(cells), host, fused, off))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write(("\n" if a.append else "") + "\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
