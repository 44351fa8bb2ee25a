"""Times transition control at 1080p beside the uniform kernels it shares a chain with, in one GPU process:

  vm_render_transition_dev                      beside vm_render_halfway_dev      (the yardstick: the product renderer)
  vm_render_transition_layers_dev, 1 and 4 ch   beside vm_render_layers_dev, 1 and 4 ch

with and without a path, device events around each call (the transition calls include whatever they launch besides the
chain).  The field is that of tools/dev_layer_warp.py (profiles/layer_warp.md); the schedule a soft diagonal wipe for
the geometry and a radial one for the colour, timed in mid-transition.  A warm-up of every call, then `--reps` rounds in
which the calls alternate; medians and minima.  The transition maps of the timed frame are compared with the statement
of tests/transit_ref.py bit for bit (what was timed is what is specified).  Writes a markdown note (default:
profiles/transition.md).  Development tool: the numbers gate nothing.

  python tools/dev_transition.py [--out PATH] [--reps N] [--size WxH]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import transit_ref as T  # noqa: E402
from videomorphing_amd import capi, morph, synth, transition  # noqa: E402

f32 = np.float32
KEYS = ("render", "transition", "layers1", "tlayers1", "layers4", "tlayers4")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transition.md"))
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--size", default="1920x1080")
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
    sg = transition.wipe(w, h, (1.0, 0.3), lead=0.6, duration=0.4)
    sk = transition.radial(w, h, None, lead=0.3, duration=0.7)
    fr = morph.Frame(ctx, w, h, ex)
    fr.upload_schedule(sg, sk)
    t, ease = 0.35, capi.EASE_SMOOTH
    rows = []
    for with_path in (False, True):
        fr.upload(morph.make_extended(rgb0, ex), morph.make_extended(rgb1, ex), v, u if with_path else None)
        ts = {k: [] for k in KEYS}
        for rep in range(a.reps + 2):                               # two rounds of warm-up
            got = {"render": fr.render_halfway_dev(t, t, 1), "transition": fr.render_transition_dev(t, ease, 1)}
            for c in (1, 4):
                fr.upload_layers(*layers[c])
                fr.render_layers_dev(t, t, 1)                       # (the first launch after an upload is not the timed one)
                got["layers%d" % c] = fr.render_layers_dev(t, t, 1)
                fr.render_transition_layers_dev(t, ease, 1)
                got["tlayers%d" % c] = fr.render_transition_layers_dev(t, ease, 1)
            if rep >= 2:
                for k in KEYS:
                    ts[k].append(got[k])
        got, want = fr.transition_maps(t, ease), T.transition_maps(v, u if with_path else None, sg, sk, t, ease)
        for g, r in zip(got, want):
            assert np.array_equal(g.view(np.uint32) if g.dtype == f32 else g, r.view(np.uint32) if r.dtype == f32 else r)
        rows.append((with_path, {k: (float(np.median(x)), float(np.min(x))) for k, x in ts.items()}, float(want[2].max()),
                     float(want[4][..., 0].min()), float(want[4][..., 0].max())))
    lines = [
        "# Transition control at %dx%d beside the uniform kernels" % (w, h),
        "",
        "Measured by `tools/dev_transition.py` on %s (%d CUs), one process, %d rounds after two of warm-up, the calls" % (name, cus, a.reps),
        "alternating within a round.  Field and path: those of `profiles/layer_warp.md`.  Schedule: a soft diagonal wipe",
        "(lead 0.6, duration 0.4) for the geometry, a radial one (lead 0.3, duration 0.7) for the colour; t = %.2f, smooth ease," % t,
        "color_from 1; the uniform calls at geo_fa = color_fa = %.2f.  Device events around each call, ms, median (minimum);" % t,
        "the transition calls include everything they launch.  `vm_render_halfway_dev` and `vm_render_layers_dev` are the",
        "kernels this change leaves as they were: the yardsticks.  The numbers gate nothing.",
        "",
        "| path | `vm_render_halfway_dev` | `vm_render_transition_dev` | `vm_render_layers_dev` 1 ch | `vm_render_transition_layers_dev` 1 ch | `vm_render_layers_dev` 4 ch | `vm_render_transition_layers_dev` 4 ch |",
        "|---|---|---|---|---|---|---|",
    ]
    for with_path, ts, resid, gmin, gmax in rows:
        lines.append("| %s | %s |" % ("yes" if with_path else "no", " | ".join("%.4f (%.4f)" % ts[k] for k in KEYS)))
    lines += ["", "Expectation (DESIGN.md 3.10, written before the run): the chain is bound by its 21 dependent taps; a third LDS read",
              "set per tap and a third staged window cost a fraction of the renderer's time, not a multiple.  Seen:", ""]
    for with_path, ts, resid, gmin, gmax in rows:
        lines.append("%s path: transition / renderer = %.2f, transition layers / layers = %.2f (1 ch), %.2f (4 ch); g of the frame spans %.3f .. %.3f, largest resid %.3g px." % (
            "With a" if with_path else "Without a", ts["transition"][0] / ts["render"][0], ts["tlayers1"][0] / ts["layers1"][0],
            ts["tlayers4"][0] / ts["layers4"][0], gmin, gmax, resid))
    lines.append("")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
